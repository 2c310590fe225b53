"""Optimiser of the reference's train loop (reference: model/net_utils.py:10-101): Rectified Adam with
the 10-slot step-size cache, the N_sma >= 5 switch and the `p -= wd*lr*p` decay applied before the Adam
update.  On the GPU every tensor of a param group is updated by ONE launch of the fused multi-tensor
kernel (`mcnerf_radam_step`, csrc/optim.hip) instead of ~10 ATen ops per tensor; the
parameters it updates are views of the flat buffers the HIP render kernels read.  Host tensors (the CPU
plumbing tests of the camera-only stage) take the same arithmetic through plain torch ops.

A param group with `"lazy_rows": True` treats the leading dimension of its tensors as rows that are optimisers of their
own: a row steps, by its own step count, only when its gradient row is not all zero (`mcnerf_radam_rows_step`, csrc/optim_rows.hip;
`RAdam._step_host_rows` on host tensors).  The default is today's dense step."""
import ctypes
import math

import torch
from torch.optim.optimizer import Optimizer

from .. import _lib


class RAdam(Optimizer):
    ROW_TABLE_CAPACITY = 1024   # first size T of a lazy group's device step-size table [T,2]; doubled whenever a step count exceeds it

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid RAdam hyper-parameter")
        self.degenerated_to_sgd = degenerated_to_sgd
        self._guard = {}            # device -> int32[2]: [0] raised by a non-finite gradient this step, [1] skipped steps so far
        self._row_tables = {}       # (group index, device) -> the step-size table of a lazy group: dict(key, T, host, table)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        buffer=[[None, None, None] for _ in range(10)], lazy_rows=False)
        super().__init__(params, defaults)
        # the cache is keyed by the step count alone, so it belongs to ONE group's betas: a group with betas of its own must not find
        # the step size of another group's beta1 in it (the one list of `defaults` would be shared by all groups)
        for group in self.param_groups:
            group["buffer"] = [[None, None, None] for _ in range(10)]

    def add_param_group(self, param_group):
        if param_group.get("lazy_rows", False):                 # the leading dimension indexes the rows: a scalar has none
            ps = param_group["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            if any(p.dim() == 0 for p in ps):
                raise ValueError("a lazy_rows param group needs tensors with a leading (row) dimension, got a 0-dim tensor")
            param_group = {**param_group, "params": ps}
        super().add_param_group(param_group)
        self.param_groups[-1]["buffer"] = [[None, None, None] for _ in range(10)]

    def load_state_dict(self, state_dict):
        """torch casts every non-"step" state tensor of a floating-point parameter to the parameter's dtype: the per-row step counts
        of a lazy group are put back as the saved int32, on the parameter's device."""
        super().load_state_dict(state_dict)
        saved = [i for g in state_dict["param_groups"] for i in g["params"]]
        mine = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(saved, mine):
            rs = state_dict["state"].get(i, {}).get("row_step")
            if rs is not None:
                self.state[p]["row_step"] = rs.to(device=p.device, dtype=torch.int32).clone()

    @staticmethod
    def _rectification(step, beta1, beta2, degenerate):
        beta2_t = beta2 ** step
        n_max = 2.0 / (1.0 - beta2) - 1.0
        n_sma = n_max - 2.0 * step * beta2_t / (1.0 - beta2_t)
        if n_sma >= 5:
            r = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2))
            return n_sma, r / (1 - beta1 ** step)
        if degenerate:
            return n_sma, 1.0 / (1 - beta1 ** step)
        return n_sma, -1.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        buckets = []            # (tensors, group, n_sma, step_size, row table | None): the fused launches of this step
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group["betas"]
            lazy = bool(group.get("lazy_rows", False))
            fused = {}          # step count -> tensors updated by one fused launch
            fused_rows = {}     # device -> tensors of a lazy group (the rows carry their own step counts)
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if lazy and "row_step" not in st:       # (a tensor that was stepped densely before goes on from its dense count)
                    st["row_step"] = torch.full((p.shape[0],), st["step"], dtype=torch.int32, device=p.device)
                st["step"] += 1
                if lazy:
                    if p.numel() == 0:
                        continue
                    if p.is_cuda:
                        fused_rows.setdefault(p.device, []).append(p)
                    else:
                        self._step_host_rows(p, p.grad, st, group, self.degenerated_to_sgd)
                    continue
                slot = group["buffer"][st["step"] % 10]
                if slot[0] != st["step"]:
                    slot[0] = st["step"]
                    slot[1], slot[2] = self._rectification(st["step"], beta1, beta2, self.degenerated_to_sgd)
                if p.is_cuda:
                    fused.setdefault(st["step"], []).append(p)
                else:
                    self._step_host(p, p.grad, st, group, slot[1], slot[2])
            for step, ps in fused.items():
                slot = group["buffer"][step % 10]
                buckets.append((ps, group, slot[1], slot[2], None))
            for dev, ps in fused_rows.items():
                buckets.append((ps, group, 0.0, 0.0, self._row_table(gi, group, dev, max(self.state[p]["step"] for p in ps))))
        # the overflow guard covers the WHOLE step: every bucket's gradients are checked before any bucket is updated, so a
        # non-finite gradient anywhere refuses the step everywhere (counted once).  (The host-side step counters have
        # advanced by then: after a refused step the bias corrections run one step ahead -- a refused step is an error
        # condition, see raise_on_overflow, not a mode of operation.  The per-row counts of a lazy group live on the device and
        # do not advance.)
        first, last = {}, {}    # (one guard per device)
        for i, b in enumerate(buckets):
            first.setdefault(b[0][0].device, i)
            last[b[0][0].device] = i
        tables = [self._bucket_tables(b[0]) for b in buckets]          # (built once: both passes use the same pointer tables)
        for i, (ps, group, n_sma, ss, _) in enumerate(buckets):        # (a lazy bucket is checked on its flat sizes)
            self._step_fused(ps, group, n_sma, ss, phase=(1 if first[ps[0].device] == i else 0) | 2, tables=tables[i])
        for i, (ps, group, n_sma, ss, rows) in enumerate(buckets):
            if rows is None:
                self._step_fused(ps, group, n_sma, ss, phase=4 | (8 if last[ps[0].device] == i else 0), tables=tables[i])
            else:
                self._step_fused_rows(ps, group, rows, count_skip=last[ps[0].device] == i, tables=tables[i])
        return loss

    def skipped_steps(self) -> int:
        """Steps the fused kernel refused because a gradient was inf / NaN (overflow of a reduced-precision mode): the
        parameters and moments of such a step are left untouched.  Synchronises; call it at epoch ends / checkpoints."""
        return int(sum(int(g[1].item()) for g in self._guard.values()))

    def raise_on_overflow(self):
        """Raises if the guard has refused steps, NAMING the weight tensors that left their precision mode's operand range
        (the packing kernels flag them per tensor: ops.range_report); with every weight in range it is an activation or a
        gradient that overflowed (f16: 65504; f16x3: activations 8188)."""
        n = self.skipped_steps()
        if n:
            from .. import ops
            bad = ops.range_report()
            if bad:
                why = "weights outside the operand range of their precision mode: " + "; ".join(
                    f"{label} {name} (mode {prec}: {ops.RANGE_TEXT[prec]})" for label, name, prec in bad)
            else:
                why = ("every packed weight is inside its mode's range, so an activation or a gradient overflowed the 16-bit operand "
                       "format (f16: 65504; f16x3: |activation| < 8188)")
            raise _lib.McnerfError(f"{n} optimiser step(s) skipped: non-finite gradients -- {why}.  Switch `precision` to 'f32' or "
                                   "lower the learning rate / add weight decay")

    @staticmethod
    def _step_host(p, g, st, group, n_sma, step_size):
        beta1, beta2 = group["betas"]
        lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
        m, v = st["exp_avg"], st["exp_avg_sq"]
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        m.mul_(beta1).add_(g, alpha=1 - beta1)
        if n_sma >= 5:
            if wd != 0:
                p.add_(p, alpha=-wd * lr)
            p.addcdiv_(m, v.sqrt().add_(eps), value=-step_size * lr)
        elif step_size > 0:
            if wd != 0:
                p.add_(p, alpha=-wd * lr)
            p.add_(m, alpha=-step_size * lr)

    @staticmethod
    @torch.no_grad()
    def _step_host_rows(p, g, st, group, degenerate=True):
        """The row-lazy rule in plain torch: the rows of `p` whose gradient row has an element != 0 advance their own
        step count st["row_step"] and take `_step_host`'s arithmetic with the step size of that count; every other row keeps its bits.
        The restatement the kernel is tested against."""
        beta1, beta2 = group["betas"]
        R = p.shape[0]
        p2, g2, m2, v2, row_step = p.view(R, -1), g.reshape(R, -1), st["exp_avg"].view(R, -1), st["exp_avg_sq"].view(R, -1), st["row_step"]
        rows = (g2 != 0).any(dim=1).nonzero().flatten()
        if rows.numel() == 0:
            return
        t = row_step[rows] + 1
        row_step[rows] = t
        for tv in t.unique().tolist():              # rows of one step count share one step size
            sel = rows[t == tv]
            n_sma, step_size = RAdam._rectification(tv, beta1, beta2, degenerate)
            sub = {"exp_avg": m2[sel], "exp_avg_sq": v2[sel]}           # (copies: gathered, updated, scattered back)
            pr = p2[sel]
            RAdam._step_host(pr, g2[sel], sub, group, n_sma, step_size)
            p2[sel], m2[sel], v2[sel] = pr, sub["exp_avg"], sub["exp_avg_sq"]

    def _row_table(self, gi, group, dev, need):
        """The device table [T,2] fp32 of a lazy group: entry t - 1 = (1.0 if N_sma(t) >= 5 else 0.0, float32(step_size(t))), T >= need.
        Entries depend on t, the betas and degenerated_to_sgd alone: built on the host by `_rectification`, copied once from pinned
        memory without blocking whenever it grows (by doubling) or its key changes, and never otherwise."""
        beta1, beta2 = group["betas"]
        key = (float(beta1), float(beta2), bool(self.degenerated_to_sgd))
        ent = self._row_tables.get((gi, dev))
        if ent is not None and ent["key"] == key and ent["T"] >= need:
            return ent
        T = ent["T"] if ent is not None and ent["key"] == key else int(self.ROW_TABLE_CAPACITY)
        while T < need:
            T *= 2
        host = torch.tensor(self._row_table_entries(T, *key), dtype=torch.float32)
        if dev.type == "cuda":
            host = host.pin_memory()
        ent = dict(key=key, T=T, host=host, table=host.to(dev, non_blocking=True))
        self._row_tables[(gi, dev)] = ent
        return ent

    @staticmethod
    def _row_table_entries(T, beta1, beta2, degenerate):
        out = []
        for t in range(1, T + 1):
            n_sma, step_size = RAdam._rectification(t, beta1, beta2, degenerate)
            out.append((1.0 if n_sma >= 5 else 0.0, step_size))
        return out

    def _bucket_tables(self, ps):
        """The device-pointer tables of one fused launch: parameters, gradients, both moments, sizes (+ the gradient tensors
        they point into, kept alive until the step's last launch)."""
        n = len(ps)
        PtrArr, SizeArr = ctypes.c_void_p * n, ctypes.c_longlong * n
        grads = []
        for p in ps:
            g = p.grad
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.McnerfError("fused RAdam needs contiguous fp32 parameters")
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
            grads.append(g)
        args = (PtrArr(*[p.data_ptr() for p in ps]), PtrArr(*[g.data_ptr() for g in grads]),
                PtrArr(*[self.state[p]["exp_avg"].data_ptr() for p in ps]),
                PtrArr(*[self.state[p]["exp_avg_sq"].data_ptr() for p in ps]),
                SizeArr(*[p.numel() for p in ps]))
        return args, grads

    def _step_fused(self, ps, group, n_sma, step_size, phase=15, tables=None):
        n = len(ps)
        args, _keep = tables if tables is not None else self._bucket_tables(ps)
        beta1, beta2 = group["betas"]
        dev = ps[0].device
        if dev not in self._guard:
            self._guard[dev] = torch.zeros(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("mcnerf_radam_step", n, *[ctypes.cast(a, ctypes.c_void_p) for a in args],
                      float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                      float(step_size), int(n_sma >= 5), self._guard[dev].data_ptr(), int(phase), torch.cuda.current_stream().cuda_stream)

    def _step_fused_rows(self, ps, group, rows, count_skip, tables):
        """The update of one lazy bucket: one launch per 64 tensors, one wave per row (csrc/optim_rows.hip)."""
        n = len(ps)
        (p_arr, g_arr, m_arr, v_arr, _sizes), _keep = tables
        PtrArr, SizeArr = ctypes.c_void_p * n, ctypes.c_longlong * n
        for p in ps:
            rs = self.state[p]["row_step"]
            if rs.dtype != torch.int32 or rs.device != p.device or rs.shape != (p.shape[0],) or not rs.is_contiguous():
                raise _lib.McnerfError("lazy_rows: state['row_step'] must be a contiguous int32 [rows] tensor on the parameter's device")
        args = (p_arr, g_arr, m_arr, v_arr, PtrArr(*[self.state[p]["row_step"].data_ptr() for p in ps]),
                SizeArr(*[p.shape[0] for p in ps]), SizeArr(*[p.numel() // p.shape[0] for p in ps]))
        beta1, beta2 = group["betas"]
        dev = ps[0].device
        with torch.cuda.device(dev):
            _lib.call("mcnerf_radam_rows_step", n, *[ctypes.cast(a, ctypes.c_void_p) for a in args],
                      float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                      rows["table"].data_ptr(), int(rows["T"]), self._guard[dev].data_ptr(), int(bool(count_skip)),
                      torch.cuda.current_stream().cuda_stream)
