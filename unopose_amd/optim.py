"""FusedAdam: the part of a training step after ``backward()`` as three HIP launches (csrc/optim.hip), gated on the device.

What the reference runs there (core/unopose/engine/engine_utils.py:53-83): ``torch.nan_to_num`` per gradient (NaN -> 0, +inf -> 1e5,
-inf -> -1e5), optionally ``clip_grad_norm_``, then ``torch.optim.Adam.step``.  ``FusedAdam.step(finite, max_norm)`` does the three in one
go over all parameters that have a gradient and returns the total gradient norm as a device scalar; nothing is read back to the host.

* ``finite``: ``None`` or a one-element bool / uint8 tensor on the parameters' device ("the loss was finite").  A clear flag turns the whole
  update off ON THE DEVICE: parameters, both moments and the step counts keep their bits.  The gradients have been cleaned by then.
* The clip coefficient multiplies the gradient inside the update; the stored gradients hold the cleaned, UNCLIPPED values afterwards
  (``clip_grad_norm_`` scales them in place -- nothing here reads them again).
* State per parameter as ``torch.optim.Adam``: ``step``, ``exp_avg``, ``exp_avg_sq``.  ``step`` is an int32 scalar on the parameter's
  device (the gate advances it there); ``state_dict()`` hands it out as the CPU float32 scalar torch's Adam keeps and
  ``load_state_dict()`` takes either, so the two optimisers read each other's checkpoints.
* A parameter whose ``.grad`` is ``None`` is left out of the step and its count does not advance (torch's rule).
* The fused route takes fp32, contiguous, GPU tensors under one set of hyper-parameters.  Anything else (CPU tensors, other dtypes, strided
  tensors, parameter groups whose hyper-parameters differ, parameters on several devices) sends the whole step through :func:`_torch_step`: the same rule, gate
  included, in torch operations.  A missing kernel is an error, not a reason to take that route."""
import numpy as np
import torch

from ._lib import call, lib, on_device, ptr, stream_ptr


def table_ints():
    """(chunk length in elements, int32 words per chunk entry, head floats of the control block, floats per tensor in it, state pointers per tensor)."""
    L = lib()
    return tuple(L.unopose_adam_table_ints(i) for i in range(5))


def chunk_table(numels, chunk, words=4):
    """The chunk entries of tensors with `numels` elements: (n_chunks, words) int32 rows [tensor, length, offset low word, offset high word] --
    tensor t cut into ceil(numel / chunk) pieces of `chunk` elements, the last one shorter; a tensor of 0 elements has no row."""
    numel = np.asarray(numels, dtype=np.int64).reshape(-1)
    count = (numel + chunk - 1) // chunk
    n_chunks = int(count.sum())
    tensor = np.repeat(np.arange(len(numel), dtype=np.int64), count)
    offset = (np.arange(n_chunks, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)) * chunk
    table = np.zeros((n_chunks, words), dtype=np.int32)
    table[:, 0] = tensor
    table[:, 1] = np.minimum(chunk, numel[tensor] - offset)
    table[:, 2:4] = offset.astype("<i8").view("<i4").reshape(n_chunks, 2)
    return table


class PinnedStaging:
    """int64 tables to the device through a ring of pinned buffers in which EVERY slot has its own event: the event is recorded behind the slot's
    copy and waited for before the slot is written again, so a loop that never synchronises cannot overwrite a table whose copy is still queued."""

    def __init__(self, slots=4):
        self.slots = [[None, None] for _ in range(slots)]  # [pinned buffer, event behind its last copy]
        self.next = 0

    def upload(self, values, dev):
        n = len(values)
        slot = self.slots[self.next % len(self.slots)]
        self.next += 1
        if slot[1] is not None:
            slot[1].synchronize()  # (long past in a steady loop: the copy was queued len(slots) uploads ago)
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(max(2 * n, 1024), dtype=torch.int64).pin_memory()
        slot[0].numpy()[:n] = values
        out = slot[0][:n].to(dev, non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(dev))
        return out


def _fusable(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.is_sparse


def _torch_step(entries, finite, max_norm):
    """The rule of the three kernels in torch operations, for tensors they do not take.  entries: (param, state, group) of the parameters that
    have a gradient.  No host read: the gate is a tensor and closes the update through torch.where."""
    dev = entries[0][0].device if entries else torch.device("cpu")
    sq = []
    for p, _, _ in entries:
        g = p.grad
        if g.is_sparse:
            raise RuntimeError("FusedAdam does not take sparse gradients")
        torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5, out=g)
        sq.append(g.detach().double().pow(2).sum().to(dev))
    norm = torch.stack(sq).sum().sqrt().float() if sq else torch.zeros((), device=dev)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm is not None else torch.ones((), device=dev)
    go = None if finite is None else finite.reshape(()).bool()
    for p, st, group in entries:
        beta1, beta2 = group["betas"]
        c, gate = coef.to(p.device), (None if go is None else go.to(p.device))
        g = p.grad.detach() * c.to(p.grad.dtype)
        if group["weight_decay"] != 0:
            g = g + group["weight_decay"] * p.detach()
        step = st["step"] + 1
        m = st["exp_avg"] + (1 - beta1) * (g - st["exp_avg"])
        v = st["exp_avg_sq"] * beta2 + ((1 - beta2) * g) * g
        t = step.double()
        step_size = (group["lr"] / (1 - beta1 ** t)).to(p.dtype)
        denom = v.sqrt() / (1 - beta2 ** t).sqrt().to(p.dtype) + group["eps"]
        new = p.detach() - step_size * (m / denom)
        for dst, val in ((p.data, new), (st["exp_avg"], m), (st["exp_avg_sq"], v), (st["step"], step)):
            dst.copy_(val if gate is None else torch.where(gate, val, dst))
    return norm


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam``'s constructor arguments (amsgrad / maximize are not offered).  ``step(finite=None, max_norm=None)`` -> total
    gradient norm (0-dim float32 tensor on the parameters' device)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError(f"FusedAdam: lr {lr}, eps {eps}, weight_decay {weight_decay} must not be negative")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: betas {betas} outside [0, 1)")
        # the keys torch.optim.Adam keeps in a parameter group, with its defaults: a state_dict of this class loads into Adam and back
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))
        self._staging = PinnedStaging()
        self._plans = {}  # gradient-set signature -> (n_chunks, chunk table, state pointer table, partials), all on the device
        self.launches = 0  # kernel launches of the last fused step (0 after a torch-route step)

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.int32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def state_dict(self):
        sd = super().state_dict()
        steps = [st["step"] for st in sd["state"].values() if "step" in st]
        host = {}
        for dev in {s.device for s in steps}:  # one copy per device, not one per parameter
            mine = [s for s in steps if s.device == dev]
            host.update(zip(map(id, mine), torch.stack(mine).cpu().tolist()))
        sd["state"] = {k: {n: (torch.tensor(float(host[id(v)]), dtype=torch.float32) if n == "step" else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] = torch.tensor(int(round(float(st["step"]))), dtype=torch.int32, device=p.device)
        self._plans.clear()

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, "_plans"):
            self._plans.clear()

    # ---- step ------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, finite=None, max_norm=None):
        entries = [(p, self._state_of(p), g) for g in self.param_groups for p in g["params"] if p.grad is not None]
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
                raise RuntimeError("FusedAdam implements amsgrad=False, maximize=False, decoupled_weight_decay=False only")
        keys = ("lr", "betas", "eps", "weight_decay")
        one_rule = all(tuple(g[k] for k in keys) == tuple(self.param_groups[0][k] for k in keys) for g in self.param_groups)
        devs = {p.device for p, _, _ in entries}
        fused = bool(entries) and one_rule and len(devs) == 1 and all(
            _fusable(p) and _fusable(p.grad) and p.grad.shape == p.shape and _fusable(st["exp_avg"]) and _fusable(st["exp_avg_sq"])
            and st["step"].dtype == torch.int32 and st["step"].device == p.device for p, st, _ in entries)
        if fused and finite is not None:
            fused = finite.device in devs and finite.numel() == 1 and finite.element_size() == 1
        if not fused:
            self.launches = 0
            return _torch_step(entries, finite, max_norm)
        return self._fused_step(entries, finite, max_norm)

    def _plan(self, entries, dev):
        sig = tuple(p.data_ptr() for p, _, _ in entries) + tuple(p.numel() for p, _, _ in entries)
        plan = self._plans.get(sig)
        if plan is None:
            chunk, words, _, _, nptr = table_ints()
            table = chunk_table([p.numel() for p, _, _ in entries], chunk, words)
            n_chunks = len(table)
            state = np.array([[p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()] for p, st, _ in entries],
                             dtype=np.int64).reshape(len(entries), nptr)
            if len(self._plans) >= 8:  # (gradient sets come and go with what a forward reaches; a run has one or two)
                self._plans.clear()
            plan = self._plans[sig] = (n_chunks, torch.from_numpy(table).to(dev), torch.from_numpy(state).to(dev),
                                       torch.empty(max(n_chunks, 1), dtype=torch.float64, device=dev))
        return plan

    def _fused_step(self, entries, finite, max_norm):
        dev = entries[0][0].device
        group = self.param_groups[0]
        beta1, beta2 = group["betas"]
        _, _, head, per_tensor, _ = table_ints()
        n = len(entries)
        with on_device(dev):
            n_chunks, chunks, state, partials = self._plan(entries, dev)
            grads = self._staging.upload([p.grad.data_ptr() for p, _, _ in entries], dev)
            block = torch.empty(head + per_tensor * n, dtype=torch.float32, device=dev)
            s = stream_ptr(dev)
            call("unopose_adam_prepare", ptr(grads), ptr(chunks), n_chunks, n, ptr(partials), s)
            call("unopose_adam_finalise", ptr(partials), n_chunks, n, ptr(state), None if finite is None else ptr(finite),
                 -1.0 if max_norm is None else float(max_norm), float(group["lr"]), float(beta1), float(beta2), ptr(block), s)
            call("unopose_adam_update", ptr(grads), ptr(state), ptr(chunks), n_chunks, n, ptr(block), float(beta1), float(beta2), float(group["eps"]),
                 float(group["weight_decay"]), s)
        self.launches = 3 if n_chunks else 1
        return block[0]
