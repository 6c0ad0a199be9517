"""Optimizers for the outer loop.  ``Adam``, ``AdamW`` and ``SGD`` are torch.optim's classes of the same names (same constructors,
``param_groups``, ``state_dict`` layouts: ``step`` / ``exp_avg`` / ``exp_avg_sq``; ``momentum_buffer``) whose ``step()`` runs as ONE
fused HIP launch over all parameter tensors when they are fp32 GPU tensors (csrc/adam.hip); any other configuration (amsgrad,
maximize, nesterov, dampening, CPU tensors, sparse grads ...) uses torch's own implementation unchanged.  ``_FusedStep`` holds what
the three share: the cached launch plans, ``step_fused`` / ``defer_step`` / ``finish_deferred`` and the bookkeeping around
``state_dict`` / pickling; a class adds its rule's flags, state tensors and launch.

``max_grad_norm=<float>`` (keyword of all three) clips the global gradient norm ahead of every step, as
``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` would: on the fused route without leaving the device and without writing
``p.grad`` (csrc/adam.hip: norm launches, finish launch, the rule on ``g * coef``); ``optimizer.clip_stats`` is the device tensor
``(norm, coef)`` of the last step.  The value lives on the optimizer object, not in ``param_groups``: ``state_dict`` stays torch's."""
import copy
import math

import torch

from . import hip

MAX_TENSORS = 32          # one fused launch (csrc/adam.hip: MAXT)
MAX_FOLDED = 24           # segments of the meta-step's final reduction (csrc/common.h: ReduceSegs)
MAX_CLIPPED = hip.MAX_CLIPPED_TENSORS      # a clipped step walks its tensors in chunks of MAX_TENSORS (csrc/adam.hip: CLIP_MAX_TENSORS)


def _checked_max_norm(v):
    if v is None:
        return None
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"max_grad_norm must be a finite number greater than 0, got {v}")
    return v


def clip_log(optimizer):
    """``{"train/grad_norm", "train/clip_coef"}`` of the last clipped step for the training loops' validation points (the one host
    read of ``clip_stats``); empty when the optimizer does not clip or has not stepped."""
    stats = getattr(optimizer, "clip_stats", None)
    if getattr(optimizer, "max_grad_norm", None) is None or stats is None:
        return {}
    norm, coef = stats.tolist()
    return {"train/grad_norm": norm, "train/clip_coef": coef}


class _FusedStep:
    """Mixed in FRONT of a torch.optim class (``_torch_cls``).  A subclass provides ``_flags_ok(group, plan)`` (the rule covers this
    group's options, and they still fit the cached plan if there is one), ``_plan(group, params, grads)`` (creates missing state
    in torch's layout and returns the cached launch arguments, or None when torch must take the step) and
    ``_launch(group, plan, device, deferred)``."""
    _torch_cls = None
    max_grad_norm = None                          # (class defaults: an optimizer pickled before the option existed has neither)
    _clip_stats = None

    @property
    def clip_stats(self):
        """Device tensor ``(norm, coef)`` of the last step taken with ``max_grad_norm`` set (None before it): the global gradient
        norm and the factor the step applied.  Reading it is the caller's host read; the step makes none."""
        return self._clip_stats

    def _torch_step(self, closure=None):
        """torch's own step, preceded by torch's own clip when ``max_grad_norm`` is set (which scales ``p.grad`` in place)."""
        if self.max_grad_norm is None:
            return self._torch_cls.step(self, closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if params:
            norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
            self._clip_stats = torch.stack([norm, torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)]).to(torch.float32)
        self._torch_cls.step(self)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._fused_args = {}                     # the state tensors were replaced: rebuild the cached pointer tables (and counts)

    def _fusable(self, group, params):
        return (params and self._flags_ok(group) and len(params) <= (MAX_TENSORS if self.max_grad_norm is None else MAX_CLIPPED)
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                        and not p.grad.is_sparse and p.grad.dtype == torch.float32 for p in params))

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            return self._torch_step(closure)
        if not self._step_impl():
            return self._torch_step()
        return None

    def step_fused(self):
        """``step()`` without torch.optim's per-call wrapper (profiler record, pre / post hook dispatch: ~8 us of host time a
        step): the models' ``evaluate`` calls this when the optimizer offers it.  Optimizer step hooks are NOT run here."""
        if self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks:
            return self.step()
        if hasattr(self.step, "_wrapped_by_lr_sched"):
            self._opt_called = True               # what the lr_scheduler's wrapper around step() records (its order check)
        with torch.no_grad():
            if not self._step_impl():
                return self._torch_step()
        return None

    def defer_step(self, device):
        """Registers this step with the device's workspace instead of launching it: the engine folds the update into the last
        launch of the training meta-step that follows (``fumi_hip_adam_step_deferred`` and its siblings; single process only --
        the caller checks).  True when registered; the caller then runs the meta-step and ``finish_deferred``.  False (nothing
        done) when the step has to go the ordinary way: first step (no gradient views yet), several groups, hooks, a
        non-fusable configuration, or ``max_grad_norm`` (the norm needs every gradient element before the first update)."""
        if self.max_grad_norm is not None:
            return False
        if self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks or len(self.param_groups) != 1:
            return False
        group = self.param_groups[0]
        cached = self._fused_args.get(0)
        params = [p for p in group["params"] if p.grad is not None]
        if cached is None or not params or len(params) > MAX_FOLDED:
            return False
        ident = tuple(p.data_ptr() for p in params) + tuple(p.grad.data_ptr() for p in params)
        if cached.ident != ident or not self._flags_ok(group, cached):
            return False
        if hasattr(self.step, "_wrapped_by_lr_sched"):
            self._opt_called = True
        self._launch(group, cached, device, True)
        return True

    def finish_deferred(self, device):
        """After the meta-step: launches the registered update on its own if the step could not fold it."""
        return hip.adam_flush(hip.Workspace.get(device), device)

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def _sync_steps(self):
        """Per-parameter ``step`` tensors (Adam's and AdamW's state layout) are brought up to date lazily: the fused launch only
        needs the count, and eight tiny tensor increments cost ~5 us of host time a step.  (SGD keeps no count.)"""
        for args in self._fused_args.values():
            lag = args.count - args.synced
            if lag:
                torch._foreach_add_(args.steps, lag)
                args.synced = args.count

    def _clip_out(self, device):
        """The optimizer's own two-float device tensor the clipped launches write (norm, coef) to."""
        t = self._clip_stats
        if t is None or t.device != device or t.dtype != torch.float32 or t.numel() != 2 or not t.is_contiguous():
            t = self._clip_stats = torch.zeros(2, device=device, dtype=torch.float32)
        return t

    def _fall_back(self):
        """torch's own step is about to run for EVERY group and will increment every `step` tensor itself: bring the tensors
        up to date and forget the cached plans, so the next fused step reads its counts from the tensors again."""
        self._sync_steps()
        self._fused_args = {}
        return False

    def __getstate__(self):
        self._sync_steps()                        # pickling / deepcopy read optimizer.state directly
        return dict(super().__getstate__(), max_grad_norm=self.max_grad_norm)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._fused_args = {}                     # (pointer tables are not pickled)

    def __deepcopy__(self, memo):
        self._sync_steps()
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, {} if k == "_fused_args" else None if k == "_clip_stats" else copy.deepcopy(v, memo))
        return new

    def _step_impl(self):
        """True when every group went through the fused launch; False (nothing done) when torch's implementation must run."""
        groups = [(g, [p for p in g["params"] if p.grad is not None]) for g in self.param_groups]
        if self.max_grad_norm is not None and len(groups) != 1:
            return self._fall_back()              # (one norm over every group: a launch per group would clip each on its own)
        plans = []
        for gi, (group, params) in enumerate(groups):
            if not params:
                continue
            grads = [p.grad for p in params]
            cached = self._fused_args.get(gi)
            # same tensors as last step (the usual case: parameters and the flat gradient views are stable): skip the checks
            ident = tuple(p.data_ptr() for p in params) + tuple(g.data_ptr() for g in grads)
            if cached is None or cached.ident != ident:
                if cached is not None:
                    self._sync_steps()            # (the replaced entry's pending count goes into the `step` tensors first)
                if not self._fusable(group, params):
                    return self._fall_back()
                cached = self._plan(group, params, grads)
                if cached is None:
                    return self._fall_back()
                self._fused_args[gi] = cached
                cached.ident = ident
                cached.dev = params[0].device
            elif not self._flags_ok(group, cached):
                return self._fall_back()
            plans.append((group, cached))
        for group, args in plans:
            self._launch(group, args, args.dev, False)
        return True


class _AdamRule(_FusedStep):
    """Adam's and AdamW's state (``step``, ``exp_avg``, ``exp_avg_sq``) and launch; they differ in the kernel's rule only."""
    _now = _later = _clipped = None

    def _flags_ok(self, group, plan=None):
        return not (isinstance(group["lr"], torch.Tensor) or group.get("amsgrad") or group.get("maximize")
                    or group.get("capturable") or group.get("differentiable"))

    def _plan(self, group, params, grads):
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)        # same layout as torch.optim.Adam
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        ms = [self.state[p]["exp_avg"] for p in params]
        vs = [self.state[p]["exp_avg_sq"] for p in params]
        plan = hip.AdamArgs(list(params), grads, ms, vs)
        plan.steps = [self.state[p]["step"] for p in params]
        plan.count = plan.synced = int(plan.steps[0])
        return plan

    def _launch(self, group, plan, device, deferred):
        plan.count += 1                                                         # (the `step` tensors follow in _sync_steps)
        b1, b2 = group["betas"]
        ws = hip.Workspace.get(device)
        if self.max_grad_norm is not None:
            type(self)._clipped(ws, plan, group["lr"], b1, b2, group["eps"], group["weight_decay"], plan.count, self.max_grad_norm,
                                self._clip_out(device), device)
        elif deferred:
            type(self)._later(ws, plan, group["lr"], b1, b2, group["eps"], group["weight_decay"], plan.count)
        else:
            type(self)._now(ws, plan, group["lr"], b1, b2, group["eps"], group["weight_decay"], plan.count, device)


class Adam(_AdamRule, torch.optim.Adam):
    _torch_cls = torch.optim.Adam
    _now, _later, _clipped = staticmethod(hip.adam_step), staticmethod(hip.adam_step_deferred), staticmethod(hip.adam_step_clipped)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self._fused_args = {}
        self.max_grad_norm = _checked_max_norm(max_grad_norm)


class AdamW(_AdamRule, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2): what --optim adamw / adamw_lin_schedule construct.  A schedule
    may rewrite ``group["lr"]`` before every step; the value is read at each launch, the deferred form included."""
    _torch_cls = torch.optim.AdamW
    _now, _later, _clipped = staticmethod(hip.adamw_step), staticmethod(hip.adamw_step_deferred), staticmethod(hip.adamw_step_clipped)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self._fused_args = {}
        self.max_grad_norm = _checked_max_norm(max_grad_norm)

    def _flags_ok(self, group, plan=None):
        return super()._flags_ok(group) and bool(group.get("decoupled_weight_decay", True))


class SGD(_FusedStep, torch.optim.SGD):
    """torch.optim.SGD with momentum (dampening 0, no Nesterov) or without.  The step that creates the momentum buffers goes
    through the fused kernel too (the buffers are written, not read); a group in which only some parameters have a buffer is
    torch's."""
    _torch_cls = torch.optim.SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kw)
        self._fused_args = {}
        self.max_grad_norm = _checked_max_norm(max_grad_norm)

    def _flags_ok(self, group, plan=None):
        return (not (isinstance(group["lr"], torch.Tensor) or group.get("nesterov") or group.get("dampening") or group.get("maximize")
                     or group.get("differentiable"))
                and (plan is None or (group["momentum"] == 0) == (plan.buf is None)))   # (momentum switched on or off: a new plan)

    def _sync_steps(self):
        pass

    def _plan(self, group, params, grads):
        bufs, first = None, False
        if group["momentum"] != 0:
            have = [self.state[p].get("momentum_buffer") is not None for p in params]
            if any(have) and not all(have):
                return None
            first = not have[0]
            # (new buffers enter optimizer.state at the launch that fills them: another group may still hand this step to torch)
            bufs = ([torch.empty_like(p, memory_format=torch.preserve_format) for p in params] if first
                    else [self.state[p]["momentum_buffer"] for p in params])
            if not all(b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() for b in bufs):
                return None
        plan = hip.SgdArgs(list(params), grads, bufs)
        plan.first = first
        plan.new_bufs = list(zip(params, bufs)) if first else None
        return plan

    def _launch(self, group, plan, device, deferred):
        ws = hip.Workspace.get(device)
        if self.max_grad_norm is not None:
            hip.sgd_step_clipped(ws, plan, group["lr"], group["momentum"], group["weight_decay"], plan.first, self.max_grad_norm,
                                 self._clip_out(device), device)
        elif deferred:
            hip.sgd_step_deferred(ws, plan, group["lr"], group["momentum"], group["weight_decay"], plan.first)
        else:
            hip.sgd_step(ws, plan, group["lr"], group["momentum"], group["weight_decay"], plan.first, device)
        if plan.first:
            for p, b in plan.new_bufs:
                self.state[p]["momentum_buffer"] = b
            plan.first, plan.new_bufs = False, None
