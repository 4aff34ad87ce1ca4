"""FlatAdam: torch.optim.Adam's step as ONE libn3dt launch over the gradient arenas (csrc/flat_adam.hip).

The reference's training step ends in two `torch.optim.Adam(...).step()` calls (talker_trainer.py:722-727 for HeadNeRFNet,
1063-1067 for Audio2style).  The gradients of both modules already live in persistent flat arenas (parallel.FlatGrads);
FlatAdam keeps `exp_avg` and `exp_avg_sq` in two more buffers of the same layout and hands the library a table of
(param, grad, exp_avg, exp_avg_sq) pointers plus a chunk list, built once per layout.  A steady-state step uploads nothing,
synchronises nothing and is one kernel launch; it is capturable in a hipGraph after one eager step.

What differs from torch.optim.Adam, on purpose:
  * all parameters of one FlatAdam share ONE step counter (a device int32).  A parameter whose `.grad` is None is skipped
    (value and state unchanged) as in torch, but the counter it will see later is the common one;
  * a step bumps the updated parameters' version counters (PyTorch's fused Adam does not), and calls
    `invalidate_packed()` on the objects passed as `modules`, so version-keyed caches of the weights are rebuilt;
  * `param_groups[g]["lr"]` stays the Python float schedulers edit; the device copy the kernel reads is refreshed by
    step() -- or by sync_hyperparameters() between replays of a captured graph, where Python does not run.

The guarded step (opt-in: `max_grad_norm=`, `skip_nonfinite=`).  With either option set, step() is two launches
(n3dt_flat_adam_guarded_step): a norm kernel over the gradients of the active tensors, then the Adam kernel.
  * total_norm = sqrt(sum g^2) over every element of every parameter whose `.grad` is not None, all groups together, on the raw
    gradient (before maximize and weight decay): what `clip_grad_norm_(params, max_norm, norm_type=2)` sees.  Squares and sums
    are formed in double in a fixed order and rounded to fp32 once, so the norm is reproducible and |g| ~ 1e30 stays finite.
  * clip_coef = min(1, max_grad_norm / (total_norm + 1e-6)) in torch's fp32 arithmetic; the Adam arithmetic sees g * clip_coef.
    `.grad` itself is NOT rewritten -- unlike clip_grad_norm_ -- which keeps the step at 4 reads + 3 writes per element.
  * skip_nonfinite=True and a total_norm that is not finite: the launch leaves every parameter, exp_avg, exp_avg_sq AND the step
    counter bit for bit as they were and adds 1 to a device-side counter.  The host does not know the outcome: version bumps
    and invalidate_packed() still happen, which costs a re-pack and nothing else.  With skip_nonfinite=False the formulas are
    evaluated as written, as torch would (a NaN norm makes the coefficient NaN).
  * `opt.grad_norm`, `opt.clip_coef` (0-dim fp32) and `opt.skipped_steps` (0-dim int32) are views of one persistent device
    record: reading the attribute synchronises nothing, and the views stay valid inside and across graph replays.  Looking at
    `skipped_steps` once per epoch replaces the reference's per-step `isnan(loss.item())`.
  * `opt.max_grad_norm` lives in that record too and is pushed by sync_hyperparameters() like the group table, so a replayed
    graph follows a change made between replays.  Whether a step is guarded at all is fixed when a graph is captured.
  * the skipped count is not part of the state dict, which stays torch.optim.Adam's.
  * data parallel: the norm is taken over what the arena holds at step() time, i.e. after GradReducer's in-place averaging, so
    every rank sees the same gradients and takes the same decision.  No collective is added.
"""
import math
import ctypes

import torch

from . import _lib, parallel

CHUNK = 4096  # elements per chunk: 256 threads x 4 vectors of 16 bytes


def arena_offsets(numels, align=parallel.FlatGrads.ALIGN):
    """Start element of every tensor in a FlatGrads-style arena (each slice starts on an `align`-element boundary) and the
    arena's total length."""
    offsets, total = [], 0
    for n in numels:
        offsets.append(total)
        total += (n + align - 1) // align * align
    return offsets, total


def build_chunks(numels, chunk=CHUNK):
    """The kernel's work list for tensors of these sizes: (tensor, start, length) triples that tile every tensor exactly
    once, in order, no chunk crossing a tensor, none longer than `chunk`.  Pure host code on sizes."""
    out = []
    for t, n in enumerate(numels):
        for s in range(0, n, chunk):
            out.append((t, s, min(chunk, n - s)))
    return out


def _step_value(s):
    v = float(s.item() if torch.is_tensor(s) else s)
    if v != int(v) or v < 0:
        raise ValueError("FlatAdam: state 'step' must be a non-negative whole number, got %r" % (v,))
    return int(v)


def unify_state(state_dict):
    """A torch.optim.Adam state dict in FlatAdam's form: {"step": int (the common counter), "state": {index: {"exp_avg",
    "exp_avg_sq"}}, "param_groups": as given}.  `step` entries may be Python numbers, CPU tensors or device tensors; they must
    all be equal -- one FlatAdam has one counter."""
    steps = {k: _step_value(v["step"]) for k, v in state_dict["state"].items()}
    if len(set(steps.values())) > 1:
        raise ValueError("FlatAdam: the loaded per-parameter 'step' values differ (%s); all parameters of one FlatAdam share "
                         "one step counter" % sorted(set(steps.values())))
    for g in state_dict["param_groups"]:
        _check_group(g)
    return {"step": next(iter(steps.values())) if steps else 0,
            "state": {k: {"exp_avg": v["exp_avg"], "exp_avg_sq": v["exp_avg_sq"]} for k, v in state_dict["state"].items()},
            "param_groups": state_dict["param_groups"]}


def torch_state(unified):
    """The inverse of unify_state: torch.optim.Adam's layout, `step` as the CPU float32 scalar tensor torch keeps."""
    return {"state": {k: {"step": torch.tensor(float(unified["step"]), dtype=torch.float32), "exp_avg": v["exp_avg"],
                          "exp_avg_sq": v["exp_avg_sq"]} for k, v in unified["state"].items()},
            "param_groups": unified["param_groups"]}


def _check_group(g):
    if g.get("amsgrad", False):
        raise ValueError("FlatAdam: amsgrad=True is not supported (the kernel keeps no max_exp_avg_sq)")
    if g.get("decoupled_weight_decay", False):
        raise ValueError("FlatAdam: decoupled_weight_decay=True (AdamW) is not supported; weight_decay is Adam's L2 term")
    if g.get("differentiable", False):
        raise ValueError("FlatAdam: differentiable=True is not supported")


def _check_max_grad_norm(v):
    if v is None:
        return None
    if torch.is_tensor(v) or isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("FlatAdam: max_grad_norm must be a Python number > 0 (inf allowed) or None (the device copy is kept by "
                         "the optimizer), got %r" % (type(v).__name__,))
    if math.isnan(v) or not v > 0:
        raise ValueError("FlatAdam: max_grad_norm must be > 0 (inf allowed), got %r" % (v,))
    return float(v)


def _bump_versions(params):
    """Move the version counters of `params` by one without a launch.  False when this PyTorch has no way to do it (then
    `modules=` is what keeps version-keyed caches right)."""
    f = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
    if f is None:
        return False
    try:
        f(params, [p._version + 1 for p in params])
    except TypeError:  # the one-tensor form of earlier releases
        for p in params:
            f(p, p._version + 1)
    return True


def _upload(dst, raw):
    """bytes -> device buffer `dst` (uint8) through a pinned staging block, stream-ordered, no synchronisation (the host
    allocator keeps the block until the copy has run)."""
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
    dst.copy_(src, non_blocking=True)


class FlatAdam(torch.optim.Optimizer):
    """Adam (amsgrad=False, L2 weight decay) whose step() is one n3dt_flat_adam_step launch.  Same constructor arguments as
    torch.optim.Adam where they apply; `modules`: objects whose invalidate_packed() is called after every step
    (HeadNeRFNet), and whose grad_arena() -- when they have one -- is the arena the state is laid out over.
    `max_grad_norm` (a Python number > 0, inf allowed) / `skip_nonfinite`: the guarded step of the module docstring -- global-norm
    clipping and non-finite step skipping on the device; both off by default, and then step() is the single launch it always was.
    fp32 CUDA parameters with dense gradients only: anything else raises, nothing falls back to PyTorch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, modules=(),
                 max_grad_norm=None, skip_nonfinite=False):
        self._max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if amsgrad:
            raise ValueError("FlatAdam: amsgrad=True is not supported (the kernel keeps no max_exp_avg_sq)")
        if torch.is_tensor(lr):
            raise ValueError("FlatAdam: lr must be a Python number (the device copy is kept by the optimizer), got a tensor")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid betas: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        # the keys torch.optim.Adam keeps in a group, so that state dicts move between the two unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        for g in self.param_groups:
            _check_group(g)
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise ValueError("FlatAdam: params must be float32, got a %s parameter of shape %s" % (p.dtype, tuple(p.shape)))
        if len(self.param_groups) > _lib.ADAM_MAX_GROUPS:
            raise ValueError("FlatAdam: at most %d param groups" % _lib.ADAM_MAX_GROUPS)
        self.modules = list(modules)
        self._ready = False
        self._has_state = False   # a step was taken or a state dict loaded (before that state_dict() has no state, as torch's)

    # ---- layout ------------------------------------------------------------------------------------------------------
    def _setup(self):
        """Resolve the arenas, allocate state, tables and counter.  Runs at the first step() / load_state_dict()."""
        for g in self.param_groups:
            for p in g["params"]:
                if not p.is_cuda:
                    raise ValueError("FlatAdam: params must live on a GPU, got a %s parameter of shape %s (there is no CPU path)"
                                     % (p.device, tuple(p.shape)))
                if not p.is_contiguous():
                    raise ValueError("FlatAdam: params must be contiguous, got strides %s for shape %s" % (p.stride(), tuple(p.shape)))
        for m in self.modules:
            if hasattr(m, "grad_arena"):
                m.grad_arena()  # (built lazily by the module's first backward otherwise: make it the layout now)
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        trainable = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
        if not trainable:
            raise ValueError("FlatAdam: no parameter requires grad")
        if len({p.device for p in trainable}) != 1:
            raise ValueError("FlatAdam: params must live on one device")
        self._device = trainable[0].device
        self._arenas = parallel._buckets_of(trainable)
        self._exp_avg = [torch.zeros_like(a.flat) for a in self._arenas]
        self._exp_avg_sq = [torch.zeros_like(a.flat) for a in self._arenas]
        # one row per tensor, arena after arena
        self._rows = [(ai, i, p) for ai, a in enumerate(self._arenas) for i, p in enumerate(a.params)]
        self._row_group = [group_of[id(p)] for _, _, p in self._rows]
        for a in self._arenas:
            assert a.offsets == arena_offsets([p.numel() for p in a.params])[0]
        self._gptr = [self._arenas[ai].flat.data_ptr() + 4 * self._arenas[ai].offsets[i] for ai, i, _ in self._rows]
        self._mptr = [self._exp_avg[ai].data_ptr() + 4 * self._arenas[ai].offsets[i] for ai, i, _ in self._rows]
        self._vptr = [self._exp_avg_sq[ai].data_ptr() + 4 * self._arenas[ai].offsets[i] for ai, i, _ in self._rows]
        chunks = build_chunks([p.numel() for _, _, p in self._rows])
        if not chunks:
            raise ValueError("FlatAdam: every parameter is empty")
        self._n_chunks = len(chunks)
        carr = (_lib.AdamChunk * len(chunks))(*[_lib.AdamChunk(s, t, n) for t, s, n in chunks])
        dev = self._device
        self._chunk_dev = torch.empty(ctypes.sizeof(carr), dtype=torch.uint8, device=dev)
        _upload(self._chunk_dev, bytes(carr))
        self._tensor_dev = torch.empty(ctypes.sizeof(_lib.AdamTensor) * len(self._rows), dtype=torch.uint8, device=dev)
        self._group_dev = torch.empty(ctypes.sizeof(_lib.AdamGroup) * len(self.param_groups), dtype=torch.uint8, device=dev)
        self._counter = torch.zeros(_lib.ADAM_COUNTER_INTS, dtype=torch.int32, device=dev)
        # the guarded step's scratch: one double per chunk, and the guard record (zero-filled once; the host writes its first
        # GUARD_HOST_BYTES from then on, the kernels the rest)
        self._partials = torch.zeros(self._n_chunks, dtype=torch.float64, device=dev)
        self._guard = torch.zeros(ctypes.sizeof(_lib.AdamGuard) // 4, dtype=torch.int32, device=dev)
        self._guard_host = self._guard[:_lib.GUARD_HOST_BYTES // 4].view(torch.uint8)
        self._guard_f32 = self._guard.view(torch.float32)
        self._pushed_guard = None
        self._pushed_tensors = None   # (param pointers, active flags) of the table on the device
        self._pushed_groups = None
        self._ready = True
        self._bind_state()

    def _bind_state(self):
        """state[p] = views of the flat buffers and the device counter (what tooling that inspects optimizer state reads)."""
        step = self._counter[0]
        for ai, i, p in self._rows:
            a = self._arenas[ai]
            sl = slice(a.offsets[i], a.offsets[i] + p.numel())
            self.state[p] = {"step": step, "exp_avg": self._exp_avg[ai][sl].view(p.shape),
                             "exp_avg_sq": self._exp_avg_sq[ai][sl].view(p.shape)}

    # ---- the guard ---------------------------------------------------------------------------------------------------
    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self._max_grad_norm = _check_max_grad_norm(v)

    @property
    def guarded(self):
        return self._max_grad_norm is not None or self.skip_nonfinite

    def _guard_field(self, name, f32):
        if not self._ready:
            self._setup()
        return (self._guard_f32 if f32 else self._guard)[getattr(_lib.AdamGuard, name).offset // 4]

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the global gradient norm of the last guarded step (a view; no synchronisation)."""
        return self._guard_field("grad_norm", True)

    @property
    def clip_coef(self):
        """0-dim fp32 device tensor: the factor the last guarded step multiplied its gradients by (a view)."""
        return self._guard_field("clip_coef", True)

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: guarded steps skipped so far for a non-finite norm (a view)."""
        return self._guard_field("skipped_steps", False)

    # ---- hyper-parameters --------------------------------------------------------------------------------------------
    def _group_values(self):
        vals = []
        for g in self.param_groups:
            _check_group(g)
            b1, b2 = g["betas"]
            vals.append((float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), int(bool(g["maximize"]))))
        return tuple(vals)

    def sync_hyperparameters(self):
        """Push lr / betas / eps / weight_decay / maximize of every group, and max_grad_norm / skip_nonfinite, to the device if
        they differ from what was last pushed (one small stream-ordered copy each, no synchronisation).  step() does this
        itself; a caller replaying a captured graph calls it between replays, after scheduler.step()."""
        if not self._ready:
            self._setup()
        vals = self._group_values()
        if vals != self._pushed_groups:
            arr = (_lib.AdamGroup * len(vals))(*[_lib.AdamGroup(*v, 0) for v in vals])
            _upload(self._group_dev, bytes(arr))
            self._pushed_groups = vals
        gvals = (0.0 if self._max_grad_norm is None else self._max_grad_norm, int(self.skip_nonfinite))
        if gvals != self._pushed_guard:
            _upload(self._guard_host, bytes(_lib.AdamGuard(*gvals))[:_lib.GUARD_HOST_BYTES])
            self._pushed_guard = gvals

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _sync_tables(self):
        """Gradients into their arena slices, then the tensor table: rebuilt only when a parameter pointer or the set of
        parameters that have a gradient changed (compared on the host)."""
        grads = [p.grad for _, _, p in self._rows]
        stray = False
        for g, gp, (ai, i, p) in zip(grads, self._gptr, self._rows):
            if g is None:
                continue
            if g.is_sparse:
                raise NotImplementedError("FlatAdam: sparse gradients are not supported (got one for a parameter of shape %s)"
                                          % (tuple(p.shape),))
            if g.data_ptr() != gp or not g.is_contiguous():
                own = getattr(p, "_n3dt_arena", None)
                if own is not None and own is not self._arenas[ai]:
                    raise RuntimeError("FlatAdam: a module rebuilt its gradient arena (a requires_grad flag or the parameter list "
                                       "changed); the optimizer state follows the old layout -- construct a new FlatAdam")
                stray = True
        if stray:
            for a in self._arenas:
                a.adopt(assign_missing=False)  # one multi-tensor copy per arena; a missing gradient stays None
        key = (tuple(p.data_ptr() for _, _, p in self._rows), tuple(g is not None for g in grads))
        if key != self._pushed_tensors:
            rows = [_lib.AdamTensor(pp, gp, mp, vp, p.numel(), gi, int(act))
                    for pp, act, gp, mp, vp, gi, (_, _, p) in zip(key[0], key[1], self._gptr, self._mptr, self._vptr, self._row_group, self._rows)]
            _upload(self._tensor_dev, bytes((_lib.AdamTensor * len(rows))(*rows)))
            self._pushed_tensors = key
        return key[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._ready:
            self._setup()
        active = self._sync_tables()
        self.sync_hyperparameters()
        if any(active):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
            if self.guarded:
                _lib.check(_lib.lib().n3dt_flat_adam_guarded_step(
                    self._tensor_dev.data_ptr(), self._chunk_dev.data_ptr(), self._n_chunks, self._group_dev.data_ptr(),
                    len(self.param_groups), self._counter.data_ptr(), self._partials.data_ptr(), self._guard.data_ptr(), stream),
                    "n3dt_flat_adam_guarded_step")
            else:
                _lib.check(_lib.lib().n3dt_flat_adam_step(self._tensor_dev.data_ptr(), self._chunk_dev.data_ptr(), self._n_chunks,
                                                          self._group_dev.data_ptr(), len(self.param_groups),
                                                          self._counter.data_ptr(), stream), "n3dt_flat_adam_step")
            self._has_state = True
            _bump_versions([p for (_, _, p), act in zip(self._rows, active) if act])
            for m in self.modules:
                if hasattr(m, "invalidate_packed"):
                    m.invalidate_packed()
        return loss

    # ---- state dicts (interchangeable with torch.optim.Adam's) -------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam's layout: state[index] = {"step" (CPU float32 scalar), "exp_avg", "exp_avg_sq"} (copies, not
        views of the flat buffers) + param_groups.  Reads the device counter once (one synchronisation; not a step-path call).
        Parameters that do not require grad have no state; before the first step there is none at all, as in torch."""
        sd = super().state_dict()
        if not (self._ready and self._has_state):
            sd["state"] = {}
            return sd
        unified = {"step": int(self._counter[0].item()), "param_groups": sd["param_groups"],
                   "state": {k: {"exp_avg": v["exp_avg"].clone(), "exp_avg_sq": v["exp_avg_sq"].clone()} for k, v in sd["state"].items()}}
        return torch_state(unified)

    def load_state_dict(self, state_dict):
        """Takes a dict saved by FlatAdam or by torch.optim.Adam over the same parameter list (the `optimizer` entry of a
        reference checkpoint).  Per-parameter steps that differ raise; parameters without state in the dict start from zeros
        at the common step."""
        unified = unify_state(state_dict)
        super().load_state_dict({"state": {}, "param_groups": unified["param_groups"]})  # groups, length checks, hooks
        for g in self.param_groups:
            if torch.is_tensor(g["lr"]):
                g["lr"] = float(g["lr"])
        if not self._ready:
            self._setup()
        else:
            self._bind_state()
        index = {}
        n = 0
        for g in self.param_groups:
            for p in g["params"]:
                index[n] = p
                n += 1
        for bufs in (self._exp_avg, self._exp_avg_sq):
            for b in bufs:
                b.zero_()
        for k, v in unified["state"].items():
            st = self.state.get(index[k])
            if st is None or "exp_avg" not in st:
                continue  # a parameter that does not require grad here
            st["exp_avg"].copy_(v["exp_avg"].to(self._device, torch.float32).view_as(st["exp_avg"]))
            st["exp_avg_sq"].copy_(v["exp_avg_sq"].to(self._device, torch.float32).view_as(st["exp_avg_sq"]))
        self._counter.copy_(torch.tensor([unified["step"]] + [0] * (_lib.ADAM_COUNTER_INTS - 1), dtype=torch.int32))
        self._has_state = True
        self._pushed_groups = None
