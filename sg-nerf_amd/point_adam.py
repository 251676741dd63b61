"""Adam on the HIP kernels: the dense fused step (sgn_adam_step_multi) and the row-sparse exact
mode for the points (sgn_adam_rows)."""
import ctypes

import torch

from . import _lib


def _check_point_tensors(names, state_dict):
    """A state written under other grad switches (another set of trained point tensors) is refused."""
    if names is None:
        return
    groups = state_dict.get("param_groups") or [{}]
    theirs = groups[0].get("point_tensors")
    if theirs is None:   # written before the switches existed: every tensor of its group trained
        if len(groups[0].get("params", ())) == len(names):
            return
        theirs = "%d unnamed tensors" % len(groups[0].get("params", ()))
    elif tuple(theirs) == tuple(names):
        return
    raise ValueError(f"point Adam state was written with trained tensors {theirs}, this optimizer trains "
                     f"{list(names)}: the feat_grad / color_grad / dir_grad / conf_grad switches differ")


class NoPointAdam:
    """The point group with every tensor frozen (feat_grad = color_grad = dir_grad = conf_grad = 0):
    nothing to step, no launch, an empty state that round-trips and refuses another switch set's."""
    rows_mode = False
    zero_grad_in_step = True
    names = ()

    def __init__(self, lr):
        self.param_groups = [{"params": [], "lr": lr, "point_tensors": []}]
        self.state = {}

    def step(self, closure=None):
        return None

    def zero_grad(self, set_to_none=True):
        pass

    def flush(self):
        pass

    def state_dict(self):
        return {"state": {}, "param_groups": [dict(self.param_groups[0], params=[])]}

    def load_state_dict(self, state_dict):
        _check_point_tensors(self.names, state_dict)
        self.param_groups[0]["lr"] = state_dict["param_groups"][0].get("lr", self.param_groups[0]["lr"])


class PointAdam(torch.optim.Adam):
    """torch.optim.Adam (same param_groups, state keys and state_dict) whose step is one
    sgn_adam_step_multi launch per parameter group; with zero_grad the launch also clears the
    gradients, so the next step skips their fill pass.  For the dense ~47 M-element point group
    and the MLP's flat parameter."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, zero_grad=True, rows=False, flush_every=256,
                 names=None, row0=True):
        """rows: row-sparse exact mode (one group of <= 4 tensors sharing their first dimension, the
        points; sgn_adam_rows).  A row is brought forward only when something reads it, replaying the
        zero-gradient steps it missed, so it equals the dense update bit for bit whenever read.  The
        step's own update is deferred to the next step's first launch: set_rows(list) applies the
        pending step to the previous step's rows and brings the new list's rows to the current step in
        one pass; flush() (state_dict, the model's renders; every flush_every steps, which bounds the
        replay) brings every row.  The narrow tensors' moments (widths <= 8, e.g. colour, dir, conf: 7
        floats a row) share one [N, 16] buffer, m in columns 0-7 and v in 8-15, and the state holds views
        of it: a row's moments are one 64-byte access instead of six scattered 4-12 byte ones.

        names: the group's tensors by name -- the trained point tensors (opt.feat_grad / color_grad /
        dir_grad / conf_grad; a frozen tensor is not in the group and has no moments).  They travel in
        the state_dict, and a state written under other names is refused.  row0: bring row 0 forward with
        every listed step (the empty neighbour slots read point 0's conf: needed while conf trains)."""
        super().__init__(params, lr=lr, betas=betas, eps=eps)
        self.names = None if names is None else tuple(names)
        if self.names is not None:
            if len(self.names) != sum(len(g["params"]) for g in self.param_groups):
                raise ValueError("PointAdam: one name per tensor")
            self.param_groups[0]["point_tensors"] = list(self.names)
        self.row0 = bool(row0)
        self.zero_grad_in_step = zero_grad
        self.rows_mode = rows
        if rows:
            ps = self.param_groups[0]["params"]
            if len(self.param_groups) != 1 or not 1 <= len(ps) <= 4:
                raise ValueError("PointAdam(rows=True): one parameter group of 1 .. 4 tensors")
            n = ps[0].shape[0]
            if any(p.shape[0] != n or not p.is_contiguous() or p.dtype != torch.float32 for p in ps):
                raise ValueError("PointAdam(rows=True): contiguous fp32 tensors sharing the first dimension")
            dev = ps[0].device
            self.n_rows = n
            widths = [p.numel() // n for p in ps]
            self._width = (ctypes.c_int32 * len(ps))(*widths)
            self._narrow, off = {}, 0   # tensor index -> its columns' offset in the packed moments
            for i, w in enumerate(widths):
                if w <= 8 and off + w <= 8:
                    self._narrow[i] = (off, w)
                    off += w
            self._mv = torch.zeros(n, 16, dtype=torch.float32, device=dev) if self._narrow else None
            self._mstride = (ctypes.c_int32 * len(ps))(*[16 if i in self._narrow else w for i, w in enumerate(widths)])
            self._last = torch.zeros(n, dtype=torch.int32, device=dev)   # the step each row holds
            self._claim = torch.zeros(n, dtype=torch.int32, device=dev)   # claim tags (launch tags start at 1)
            self._claim2 = torch.zeros(n, dtype=torch.int32, device=dev)
            self._sched = torch.zeros(2 * 1024, dtype=torch.float32, device=dev)
            self._ws = None
            self._pend = [None, None]   # two pend lists: the previous step's is read while the next is written
            self._pi = 0
            self._tag = 0
            self._rows = None           # the step's list (set_rows) once its rows are brought forward
            self._pending = None        # (pend buffer, length bound): the rows of the step not yet applied
            self._flushed = 0           # every row holds at least this step
            self.flush_every = flush_every

    # -- row-sparse mode ------------------------------------------------------------------------
    def _state_step(self):
        """The group's step count (0 before the first step); creates the state tensors."""
        for i, p in enumerate(self.param_groups[0]["params"]):
            s = self.state[p]
            if not s:
                s["step"] = torch.tensor(0.0)
                if i in self._narrow:
                    s["exp_avg"], s["exp_avg_sq"] = self._mv_views(i)
                else:
                    s["exp_avg"] = torch.zeros_like(p)
                    s["exp_avg_sq"] = torch.zeros_like(p)
        return int(self.state[self.param_groups[0]["params"][0]]["step"].item())

    def _mv_views(self, i):
        """Tensor i's exp_avg / exp_avg_sq as views of the packed narrow moments (zero at creation)."""
        o, w = self._narrow[i]
        return self._mv[:, o:o + w], self._mv[:, 8 + o:8 + o + w]

    def _buf(self, t, nbytes):
        if t is None or t.numel() < nbytes:
            t = torch.empty(nbytes, dtype=torch.uint8, device=self._last.device)
        return t

    def _launch(self, step, apply, rows=None, count=None, count_is64=False, count_mul=1, n_max=None, pend=False,
                lr=None):
        """One sgn_adam_rows call: list 1 (rows, or every row), the pending list as list 2 when applying a
        deferred step, row 0; with pend, list 1's distinct rows go to the next pend buffer."""
        g = self.param_groups[0]
        ps = g["params"]
        n = len(ps)
        arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
        if step >= self._sched.numel() // 2:   # grow the per-step constant table (entries kept)
            grown = torch.zeros(max(2 * self._sched.numel(), 2 * (step + 1)), dtype=torch.float32,
                                device=self._sched.device)
            grown[:self._sched.numel()] = self._sched
            self._sched = grown
        b1, b2 = g["betas"]
        self._tag = (self._tag + 1) & 0x7fffffff
        n_max = self.n_rows if n_max is None else n_max
        L = _lib.lib()
        prev = self._pending if apply and rows is not None else None
        lr = float(g["lr"]) if lr is None else lr
        n2 = prev[1] if prev is not None else 0
        self._ws = self._buf(self._ws, int(L.sgn_adam_rows_workspace_bytes(min(n_max + n2 + 1, self.n_rows))))
        pb = None
        if pend:
            self._pi ^= 1
            pb = self._pend[self._pi] = self._buf(self._pend[self._pi],
                                                  int(L.sgn_adam_rows_pend_bytes(min(n_max + 1, self.n_rows))))
        _lib.check(L.sgn_adam_rows(
            n, arr(ps), arr([p.grad if apply else None for p in ps]), arr([self.state[p]["exp_avg"] for p in ps]),
            arr([self.state[p]["exp_avg_sq"] for p in ps]), self._width, self._mstride, self.n_rows,
            _lib.ptr(rows) if rows is not None else None, _lib.ptr(count) if count is not None else None,
            int(count_is64), count_mul, n_max, int(self.row0),
            prev[0].data_ptr() + 16 if prev is not None else None, prev[0].data_ptr() if prev is not None else None,
            n2, _lib.ptr(self._last), _lib.ptr(self._claim), _lib.ptr(self._claim2), self._tag,
            _lib.ptr(self._ws), self._ws.numel(), _lib.ptr(pb) if pb is not None else None,
            pb.numel() if pb is not None else 0, _lib.ptr(self._sched), lr, b1, b2, float(g["eps"]),
            step, int(apply), int(self.zero_grad_in_step), _lib.stream_handle()), "sgn_adam_rows")
        return pb

    def set_rows(self, rows, count=None, count_is64=False, count_mul=1, n_max=None):
        """The rows the coming step reads and changes: an int32 device list (-1 / duplicates allowed)
        with its device count (int32 or int64, times count_mul) or host length n_max.  One launch
        applies the deferred previous step to its rows and brings these rows (and row 0) to the current
        step; returns the step's distinct rows (int32 from byte 16 of the returned buffer, int64 count
        at byte 0, list-1 ids >= n_rows at byte 8)."""
        assert self.rows_mode and rows.dtype == torch.int32 and rows.is_contiguous()
        n_max = rows.numel() if n_max is None else n_max
        t = self._state_step()
        pd = self._pending
        pb = self._launch(t, apply=pd is not None, rows=rows, count=count, count_is64=count_is64,
                          count_mul=count_mul, n_max=n_max, pend=True, lr=pd[2] if pd is not None else None)
        self._pending = None
        self._rows = (pb, min(n_max + 1, self.n_rows))
        return pb

    def set_update_rows(self, rows):
        """Under DP: the rows the step's update changes (every rank's, int32 device, host length) --
        they replace the step's pend list (a launch gathers their distinct rows now)."""
        assert self.rows_mode and rows.dtype == torch.int32 and rows.is_contiguous()
        t = self._state_step()
        pb = self._launch(t, apply=False, rows=rows, n_max=rows.numel(), pend=True)
        self._rows = (pb, min(rows.numel() + 1, self.n_rows))

    @torch.no_grad()
    def flush(self):
        """Bring every row to the current step (before anything outside the step reads the tensors)."""
        if not self.rows_mode:
            return
        t = self._state_step()
        pd = self._pending
        if pd is not None or t > self._flushed:
            self._launch(t, apply=pd is not None, lr=pd[2] if pd is not None else None)
            self._pending = None
            self._flushed = t

    def state_dict(self):
        self.flush()
        return super().state_dict()

    def zero_grad(self, set_to_none=True):
        """A deferred step reads its gradient at the next launch: apply it before the gradient goes."""
        if self.rows_mode and self._pending is not None:
            self.flush()
        super().zero_grad(set_to_none)

    def load_state_dict(self, state_dict):
        _check_point_tensors(self.names, state_dict)
        super().load_state_dict(state_dict)
        if self.rows_mode:   # the loaded tensors are a dense state: every row holds its step
            for i, p in enumerate(self.param_groups[0]["params"]):
                s = self.state[p]
                if i in self._narrow and s:   # back into the packed moments
                    for key, view in zip(("exp_avg", "exp_avg_sq"), self._mv_views(i)):
                        view.copy_(s[key].reshape(view.shape))
                        s[key] = view
            t = self._state_step()
            self._last.fill_(t)
            self._flushed = t
            self._pending = None
            self._rows = None

    @torch.no_grad()
    def step(self, closure=None):
        """One sgn_adam_step_multi launch per parameter group (tensors sharing a step count); in the
        row-sparse mode the step is recorded as pending on the rows set_rows listed (applied by the next
        set_rows or flush), or applied to every row at once without such a list."""
        assert closure is None
        if self.rows_mode:
            if self._pending is not None:   # the previous step was never applied: its gradient is this one
                self.flush()
            t = self._state_step() + 1
            for p in self.param_groups[0]["params"]:
                self.state[p]["step"] += 1
            r = self._rows
            self._rows = None
            if r is None:
                self._launch(t, apply=True)
                self._flushed = t
            else:   # the step's lr travels with it: the update runs at the next set_rows / flush
                self._pending = (r[0], r[1], float(self.param_groups[0]["lr"]))
                if t - self._flushed >= self.flush_every:
                    self.flush()
            return None
        L = _lib.lib()
        st = _lib.stream_handle()
        for g in self.param_groups:
            b1, b2 = g["betas"]
            by_step = {}
            for p in g["params"]:
                if p.grad is None:
                    continue
                assert p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32
                s = self.state[p]
                if not s:
                    s["step"] = torch.tensor(0.0)
                    s["exp_avg"] = torch.zeros_like(p)
                    s["exp_avg_sq"] = torch.zeros_like(p)
                s["step"] += 1
                by_step.setdefault(int(s["step"].item()), []).append(p)
            for step, ps in by_step.items():
                for i in range(0, len(ps), 8):
                    chunk = ps[i:i + 8]
                    n = len(chunk)
                    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
                    _lib.check(L.sgn_adam_step_multi(
                        n, arr(chunk), arr([p.grad for p in chunk]), arr([self.state[p]["exp_avg"] for p in chunk]),
                        arr([self.state[p]["exp_avg_sq"] for p in chunk]), (ctypes.c_int64 * n)(*[p.numel() for p in chunk]),
                        float(g["lr"]), b1, b2, float(g["eps"]), step, int(self.zero_grad_in_step), st),
                        "sgn_adam_step_multi")
        return None
