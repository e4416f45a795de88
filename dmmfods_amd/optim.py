"""Flat fused Adam over the model's parameter arena (reference: torch.optim.Adam built at
agents/Dense_U_Net_lidar_Agent.py:57-61 and stepped at :265).  One kernel launch updates every parameter;
state_dict()/load_state_dict() use torch.optim.Adam's layout so reference checkpoints round-trip.

New here (the reference trains in fp32 with a bare Adam): the GUARDED step - a dynamic loss scale (torch.amp.GradScaler's rule),
a skipped step when the gradient arena holds an inf or a NaN, and clipping by the global gradient norm
(torch.nn.utils.clip_grad_norm_'s formula).  ``FusedAdam(model, max_grad_norm=..., loss_scaler=DynamicLossScaler())`` turns it
on; everything is decided on the device (include/dmmfods_hip.h, dmm_adam_step_guarded), so step() never waits for the GPU.

Gradient accumulation (model.set_grad_accumulation(True)): zero_grad() clears the arena at the start of a window, every backward
of the window adds into it, step() closes it.  Neither step changes.  The guarded step reduces over the arena as stored, and the
dynamic scale S changes only inside step(), so it is constant over a window: the arena holds S x sum_i g_i, the norm that is
clipped is that of the summed gradient, and one non-finite micro-batch leaves an inf / NaN in the sum - the WHOLE window's step is
then skipped and S backs off once.

Parameter groups (``FusedAdam(model, param_groups=[...])``, as torch.optim.Adam takes them: the released encoder at a lower learning
rate than the decoder, no weight decay on BatchNorm weights and biases - ``fine_tune_groups``) and decoupled weight decay
(``decoupled_weight_decay=True``: AdamW's rule).  Groups interleave tensor by tensor in the arena, so the step is ONE launch of the
segmented kernel (dmm_adam_step_segmented / dmm_adam_step_guarded_segmented) under a device table of (begin, count, class)
segments; a class is a (group, step origin) pair and carries its hyper-parameters with every call.  An optimiser without
either keyword is an optimiser with one group: while nothing is or was frozen its step is the whole-arena call (dmm_adam_step /
dmm_adam_step_guarded: the same kernel without a table), with a frozen or released encoder it is the same one launch under a table.

Parameter average (``FusedAdam(model, ema_decay=0.999)``; the reference has none and picks its best checkpoint on the raw iterate,
A:165-213): an exponential moving average of the trainable parameters, kept by the SAME Adam launch (dmm_adam_step_segmented_ema /
dmm_adam_step_guarded_segmented_ema) from the new parameter each thread holds in registers: e += (1 - d_k) (p - e) wherever the step
wrote p - not on a skipped step, not in a frozen range (there e == p holds, and a released range simply joins).  d_k = decay, or with
``ema_warmup`` (the default) min(decay, (1 + k) / (10 + k)) at the k-th averaging update (TF's ExponentialMovingAverage with
num_updates).  ``ema_arena`` holds it, ``with opt.ema_weights():`` runs the model on it, ``ema_state_dict()`` exports it.  The BatchNorm
running statistics and num_batches_tracked are NOT averaged: the live ones are used (TF's ema.apply(trainable_variables) convention)."""
import collections
import contextlib
import ctypes as C
import math
import numbers

import torch

from . import _lib

_STATE_KEY = "loss_scaler"   # the one extra top-level key of FusedAdam.state_dict() on the guarded path
_EMA_KEY = "ema"             # and the one of an optimiser that keeps a parameter average


class DynamicLossScaler:
    """Dynamic loss scale S with torch.amp.GradScaler's rule and defaults.  The loss kernel multiplies d(loss)/d(logit) by S
    (on top of the model's static ``loss_scale``), so the gradient arena holds S x the gradients; the optimiser divides it out.
    A step whose arena holds an inf / NaN is skipped: parameters, moments and the optimiser's step count stay, S *= backoff_factor.
    After ``growth_interval`` applied steps in a row S *= growth_factor; ``growth_interval=0``: S never grows (it still backs off).
    S may fall below 1.  As with torch.amp, the forward of a skipped step has already updated the BatchNorm running statistics and
    ``num_batches_tracked``.

    The state (dmm_guard_state: scale, counters, the last step's norm and flag) lives in one 64-byte device block that is created
    on the model's device when first needed; reading ``get_scale()``, ``skipped_steps`` or ``state_dict()`` waits for the GPU, the
    device tensors ``loss_scale`` / ``last_grad_norm`` / ``last_found_inf`` do not."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not (math.isfinite(init_scale) and init_scale > 0):
            raise ValueError("init_scale must be a finite number > 0")
        if not (math.isfinite(growth_factor) and growth_factor > 1):
            raise ValueError("growth_factor must be > 1")
        if not 0 < backoff_factor < 1:
            raise ValueError("backoff_factor must lie in (0, 1)")
        if int(growth_interval) != growth_interval or growth_interval < 0:
            raise ValueError("growth_interval must be an integer >= 0 (0: the scale never grows)")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._fixed = False
        self._reset(float(init_scale))

    @classmethod
    def _fixed_unit(cls):
        """S = 1 for ever: the state block of a FusedAdam that clips (or only guards) without a loss scale."""
        s = cls.__new__(cls)
        s.growth_factor, s.backoff_factor, s.growth_interval = 1.0, 1.0, 0
        s._fixed = True
        s._reset(1.0)
        return s

    def _reset(self, scale):
        self._host = {"scale": scale, "growth_tracker": 0, "skipped_steps": 0, "applied_steps": 0}   # valid while _state is None
        self._state = None        # int32[16] = dmm_guard_state
        self._skipped_base = 0    # skipped steps before the device block was (re)initialised
        self._scratch = None

    # ---- the device block ----
    def _views(self):
        s = self._state
        return s.view(torch.float32), s.view(torch.int64), s.view(torch.float64)

    def _push(self):
        """(Re)initialise the device block from the host values."""
        h, dev = self._host, self._state.device
        _lib.check(_lib.lib().dmm_guard_state_init(self._state.data_ptr(), float(h["scale"]), int(h["applied_steps"]),
                                                   int(h["growth_tracker"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self._skipped_base = int(h["skipped_steps"])

    def _pull(self):
        """Host copy of the counters (waits for the GPU)."""
        if self._state is not None:
            raw = self._state.cpu()
            f, i64 = raw.view(torch.float32), raw.view(torch.int64)
            self._host = {"scale": float(f[0]), "growth_tracker": int(raw[10]), "skipped_steps": self._skipped_base + int(i64[4]),
                          "applied_steps": int(i64[3])}
        return self._host

    def _materialize(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the loss scaler's state lives on the GPU (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._state is not None and self._state.device == device:
            return self._state
        self._pull()
        self._state = torch.zeros(16, dtype=torch.int32, device=device)
        self._scratch = None
        self._push()
        return self._state

    def _scale_ptr(self, device):
        return self._materialize(device).data_ptr()   # `scale` is the block's first field

    def _scratch_for(self, n):
        nbytes = _lib.lib().dmm_grad_guard_scratch_bytes(int(n))
        if self._scratch is None or self._scratch.device != self._state.device or self._scratch.numel() * 8 < nbytes:
            self._scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=self._state.device)
        return self._scratch

    def _set_applied(self, n):
        self._host["applied_steps"] = int(n)
        if self._state is not None:
            self._views()[1][3:4].fill_(int(n))

    def _applied(self):
        return int(self._views()[1][3]) if self._state is not None else int(self._host["applied_steps"])

    # ---- public surface ----
    @property
    def loss_scale(self):
        """Device tensor (1 element): the scale of the next backward.  None until the state exists on a device."""
        return None if self._state is None else self._views()[0][0:1]

    @property
    def last_grad_norm(self):
        """Device tensor: global gradient norm of the last step, unscaled, before clipping (inf / NaN when it was skipped)."""
        return None if self._state is None else self._views()[0][4:5]

    @property
    def last_found_inf(self):
        """Device tensor (int32): 1 when the last step was skipped."""
        return None if self._state is None else self._state[5:6]

    @property
    def last_clip_coef(self):
        return None if self._state is None else self._views()[0][13:14]

    def get_scale(self):
        return float(self._pull()["scale"])

    def set_scale(self, scale):
        """Rewrite the scale (on the device, without waiting for it); the counters stay."""
        if not (math.isfinite(scale) and scale > 0):
            raise ValueError("scale must be a finite number > 0")
        self._host["scale"] = float(scale)
        if self._state is not None:
            self._views()[0][0:1].fill_(float(scale))

    @property
    def skipped_steps(self):
        return int(self._pull()["skipped_steps"])

    @property
    def growth_tracker(self):
        return int(self._pull()["growth_tracker"])

    def state_dict(self):
        h = self._pull()
        return {"scale": float(h["scale"]), "growth_tracker": int(h["growth_tracker"]), "skipped_steps": int(h["skipped_steps"])}

    def load_state_dict(self, sd):
        applied = self._applied()
        scale, tracker = (1.0, 0) if self._fixed else (float(sd["scale"]), int(sd.get("growth_tracker", 0)))
        if not (math.isfinite(scale) and scale > 0) or tracker < 0:
            raise ValueError("bad loss scaler state")
        self._host = {"scale": scale, "growth_tracker": tracker, "skipped_steps": int(sd.get("skipped_steps", 0)), "applied_steps": applied}
        if self._state is not None:
            self._push()


class FusedAdam:
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, max_grad_norm=None,
                 loss_scaler=None, param_groups=None, decoupled_weight_decay=False, ema_decay=None, ema_warmup=True):
        """ema_decay: None (no average: nothing of it exists and state_dict() has no "ema" key) or a number in [0, 1).  It is held as
        the fp32 value the C ABI carries, so that ema_decay_at() is what the kernel uses.  ema_warmup: see ema_decay_at()."""
        if amsgrad:
            raise ValueError("amsgrad=True is not supported (reference default False, H:156)")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0 and math.isfinite(float(max_grad_norm))):
            raise ValueError("max_grad_norm must be a finite number > 0 (None: no clipping)")
        if loss_scaler is not None and not isinstance(loss_scaler, DynamicLossScaler):
            raise ValueError("loss_scaler must be a DynamicLossScaler")
        if ema_decay is not None:
            if not isinstance(ema_decay, numbers.Real) or isinstance(ema_decay, bool):
                raise ValueError("ema_decay must be None or a number in [0, 1)")
            ema_decay = C.c_float(float(ema_decay)).value
            if not 0.0 <= ema_decay < 1.0:   # (NaN fails both)
                raise ValueError("ema_decay must lie in [0, 1) (as an fp32 value)")
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.model = model
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False)
        self._params = list(model.parameters())
        # An optimiser without param_groups is an optimiser with one group.  _grouped only says which checkpoint format it keeps:
        # without either keyword the groups carry no "decoupled_weight_decay" key, betas stay as loaded, and segments() is None.
        self._grouped = param_groups is not None or bool(decoupled_weight_decay)
        if self._grouped:
            self.defaults["decoupled_weight_decay"] = bool(decoupled_weight_decay)
            self._build_groups(param_groups)
        else:
            self.param_groups = [dict(self.defaults, params=list(range(len(self._params))))]
            self._torch_index = list(range(len(self._params)))   # arena position -> torch's parameter number
            self._group_of = [0] * len(self._params)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.loss_scaler = loss_scaler
        # the guarded path's state block: the scaler's, or a private S = 1 one for clipping alone; None = the plain step
        self._guard = loss_scaler if loss_scaler is not None else (DynamicLossScaler._fixed_unit() if max_grad_norm is not None else None)
        self._step_count = 0
        if loss_scaler is not None:
            model.set_loss_scaler(loss_scaler)
        self._alloc()
        # Per-parameter step origins (torch.optim.Adam counts steps per parameter): _t0[i] is the applied-step count at which
        # parameter i began to train (its Adam step is count - _t0[i]); None: never trainable so far (no state, as in torch).
        # _frozen_at[i]: the count at which a parameter that has trained was frozen (None: trainable now, or never trained).
        self._t0 = [0 if p.requires_grad else None for p in self._params]
        self._frozen_at = [None] * len(self._params)
        self._sig = tuple(p.requires_grad for p in self._params)
        self._ranges = None
        self._model_sig = None   # the model's own record of the flags (an object replaced on every change) when _ranges was built
        # [begin, count, class] over the arena, the (group, t0) of every class, and the device table built from them
        self._segments = self._classes = self._table = None
        # The parameter average: plain path - _ema_k averaging updates so far, counted here; guarded path - only the applied-step
        # count at which averaging began (_ema_t0): the device knows which steps were applied.
        self.ema_arena = None
        self._ema_k = self._ema_t0 = 0
        self._ema_swapped = False
        if self.ema_decay is not None:
            self.ema_reset()

    _GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay")

    def _build_groups(self, param_groups):
        """self.param_groups in torch's form: the live dicts, "params" = torch's numbers (consecutive through the groups, in group
        order).  Every parameter of the model lies in exactly one group."""
        if param_groups is None:
            param_groups = [{"params": list(self._params)}]
        param_groups = list(param_groups)
        if not param_groups or not all(isinstance(g, dict) and "params" in g for g in param_groups):
            raise ValueError("param_groups must be a non-empty list of dicts with a 'params' entry")
        where = {id(p): i for i, p in enumerate(self._params)}
        self._torch_index = [None] * len(self._params)
        self._group_of = [None] * len(self._params)
        self.param_groups, k = [], 0
        for gi, g in enumerate(param_groups):
            # (torch.optim.Adam writes its defaults into the dicts it is given: a list that went through it carries these keys)
            unknown = set(g) - set(self._GROUP_KEYS) - {"params", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused"}
            if unknown:
                raise ValueError(f"param group {gi}: unknown key {sorted(unknown)[0]!r}")
            if g.get("amsgrad"):
                raise ValueError("amsgrad=True is not supported (reference default False, H:156)")
            if g.get("maximize"):
                raise ValueError("maximize=True is not supported")
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            if not ps:
                raise ValueError(f"param group {gi} is empty")
            own = dict(self.defaults, **{key: g[key] for key in self._GROUP_KEYS if key in g})
            own["betas"] = tuple(own["betas"])
            own["decoupled_weight_decay"] = bool(own["decoupled_weight_decay"])
            own["params"] = []
            for p in ps:
                i = where.get(id(p)) if isinstance(p, torch.Tensor) else None
                if i is None:
                    raise ValueError(f"param group {gi} holds a tensor that is not a parameter of the model")
                if self._group_of[i] is not None:
                    raise ValueError(f"parameter {i} of the model appears in more than one parameter group ({self._group_of[i]} and {gi})")
                self._group_of[i], self._torch_index[i] = gi, k
                own["params"].append(k)
                k += 1
            self.param_groups.append(own)
        missing = [i for i, g in enumerate(self._group_of) if g is None]
        if missing:
            raise ValueError(f"parameter {missing[0]} of the model is in no parameter group ({len(missing)} are missing): every parameter "
                             "must be in exactly one")
        if len(self.param_groups) > _lib.ADAM_MAX_CLASSES:
            raise ValueError(f"{len(self.param_groups)} parameter groups: the segmented step carries at most {_lib.ADAM_MAX_CLASSES} classes")

    # ---- trainable ranges ----
    def _sync_trainable(self, look=True):
        """Rebuilds the step origins and the range list when the model's trainable set has changed since the last look.  Reads the
        applied-step count: on the guarded path that is ONE wait for the device, at a rare event (freezing or releasing the
        encoder).  look=False (step()): the flags are not read again while the model's record of them - renewed by
        freeze_encoder() and by every training-mode forward that finds a flag changed - is the object this list was built from;
        a requires_grad_() set directly between a backward and its step() is therefore honoured from the next forward on, which is
        also when the gradients begin to match it."""
        msig = getattr(self.model, "_trainable_sig", None)
        if not look and msig is not None and msig is self._model_sig and self._ranges is not None:
            return
        if look and hasattr(self.model, "_check_trainable_set"):
            self.model._check_trainable_set()   # validates the set, closes plans of the other mode
            msig = self.model._trainable_sig
        sig = tuple(p.requires_grad for p in self._params)
        self._model_sig = msig
        if sig == self._sig and self._ranges is not None:
            return
        if sig != self._sig:
            count = self.step_count
            for i, (now, was) in enumerate(zip(sig, self._sig)):
                if now and not was:      # released: a first-time parameter starts at step 1; one that trained before goes on where it was
                    if self._t0[i] is None:
                        self._t0[i] = count
                    elif self._frozen_at[i] is not None:
                        self._t0[i] += count - self._frozen_at[i]
                    self._frozen_at[i] = None
                elif was and not now and self._t0[i] is not None:
                    self._frozen_at[i] = count
            self._sig = sig
        self._ranges = []
        off = 0
        for i, p in enumerate(self._params):
            n = p.numel()
            if sig[i]:
                last = self._ranges[-1] if self._ranges else None
                if last is not None and last[0] + last[1] == off and last[2] == self._t0[i]:
                    last[1] += n
                else:
                    self._ranges.append([off, n, self._t0[i]])
            off += n
        if not self._ranges:
            raise ValueError("no parameter of the model is trainable")
        self._build_segments(sig)

    def _build_segments(self, sig):
        """The segment list of the trainable set: a class is a (group, step origin) pair, adjacent tensors of one class merge.  The
        device table is built from it at the next step (it needs the arena's device); hyper-parameters are not part of it."""
        classes, segs, off = {}, [], 0
        for i, p in enumerate(self._params):
            n = p.numel()
            if sig[i] and n:
                c = classes.setdefault((self._group_of[i], self._t0[i]), len(classes))
                if segs and segs[-1][0] + segs[-1][1] == off and segs[-1][2] == c:
                    segs[-1][1] += n
                else:
                    segs.append([off, n, c])
            off += n
        if len(classes) > _lib.ADAM_MAX_CLASSES:
            self._ranges = None   # (nothing half-built is kept: the next look raises again)
            raise ValueError(f"{len(classes)} (parameter group, step origin) classes: the segmented step carries at most {_lib.ADAM_MAX_CLASSES}")
        self._segments, self._classes, self._table = segs, list(classes), None

    def segments(self):
        """[(begin, count, group, t0)]: the segments of the grouped step (elements of the arena), None without groups."""
        self._sync_trainable()
        if not self._grouped:
            return None
        return [(b, n, *self._classes[c]) for b, n, c in self._segments]

    def _ensure_table(self):
        """The device form of the segment list (dmm_adam_table_init), rebuilt when the trainable set or the arena's device changed."""
        dev = self.model.param_arena.device
        if self._table is not None and self._table.device == dev:
            return self._table
        L, n, k = _lib.lib(), self.model.param_arena.numel(), len(self._segments)
        segs = (_lib.AdamSegment * k)(*(_lib.AdamSegment(b, c, cls) for b, c, cls in self._segments))
        table = torch.empty((L.dmm_adam_table_bytes(k, n) + 7) // 8, dtype=torch.int64, device=dev)
        _lib.check(L.dmm_adam_table_init(table.data_ptr(), segs, k, n, len(self._classes), _lib.stream_ptr()))
        self._table = table
        return table

    def _class_array(self):
        """The classes of this step, by value: the groups' hyper-parameters as they are NOW (a scheduler writes g["lr"])."""
        out = (_lib.AdamClass * len(self._classes))()
        for k, (gi, t0) in enumerate(self._classes):
            g = self.param_groups[gi]
            out[k] = _lib.AdamClass(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                                    1 if g.get("decoupled_weight_decay") else 0, int(t0))
        return out

    def trainable_ranges(self):
        """[(offset, count, t0)]: the contiguous trainable runs of the arena (elements), each with the applied-step count at which it
        became trainable (0: from the start).  Adjacent runs with different origins stay apart."""
        self._sync_trainable()
        return [tuple(r) for r in self._ranges]

    def _param_step(self, i, count):
        """Parameter i's own Adam step count (0: no state yet)."""
        if self._t0[i] is None:
            return 0
        end = count if self._frozen_at[i] is None else self._frozen_at[i]
        return max(0, end - self._t0[i])

    def _alloc(self):
        p = self.model.param_arena
        self.exp_avg = torch.zeros_like(p)
        self.exp_avg_sq = torch.zeros_like(p)

    @property
    def step_count(self):
        """Optimiser steps APPLIED so far.  On the guarded path the count lives on the device (a skipped step does not count) and
        reading it waits for the GPU; step() itself never does."""
        if self._guard is not None:
            return self._guard._applied()
        return self._step_count

    @step_count.setter
    def step_count(self, n):
        self._step_count = int(n)
        if self._guard is not None:
            self._guard._set_applied(int(n))

    # device tensors for logging without a synchronisation (None on the plain path / before the first guarded step)
    @property
    def last_grad_norm(self):
        return None if self._guard is None else self._guard.last_grad_norm

    @property
    def last_found_inf(self):
        return None if self._guard is None else self._guard.last_found_inf

    @property
    def loss_scale(self):
        return None if self._guard is None else self._guard.loss_scale

    def zero_grad(self, set_to_none=False):
        """By default the HIP backward overwrites the gradient arena, so there is nothing to clear (kept for API parity).  While
        the model accumulates gradients (set_grad_accumulation(True)) the arena is zeroed, in stream order on the current stream
        and without waiting for the device; ``set_to_none`` is ignored (.grad are views of the arena)."""
        if getattr(self.model, "grad_accumulation", False):
            self.model.grad_arena.zero_()

    # ---- the parameter average ----
    def _ema_need(self):
        if self.ema_arena is None:
            raise RuntimeError("this optimiser keeps no parameter average (ema_decay=None)")

    def _ema_follow(self):
        if self.ema_arena.device != self.model.param_arena.device:
            self.ema_arena = self.ema_arena.to(self.model.param_arena.device)

    @torch.no_grad()
    def ema_reset(self):
        """The average starts again: a copy of the parameters as they are now, and the next step is averaging update 1.  (On the
        guarded path this reads the applied-step count, i.e. waits for the device.)"""
        if self.ema_decay is None:
            raise RuntimeError("this optimiser keeps no parameter average (ema_decay=None)")
        if self._ema_swapped:
            raise RuntimeError("ema_reset() inside ema_weights(): the parameter arena holds the average")
        self.ema_arena = self.model.param_arena.detach().clone()
        self._ema_k = 0
        self._ema_t0 = self.step_count if self._guard is not None else 0

    @property
    def ema_num_updates(self):
        """Averaging updates so far.  On the guarded path the count of applied steps lives on the device: reading this waits for
        the GPU, as step_count does."""
        self._ema_need()
        return max(0, self.step_count - self._ema_t0) if self._guard is not None else self._ema_k

    def ema_decay_at(self, k):
        """d_k of averaging update k >= 1, in double: ema_decay, or with ema_warmup min(ema_decay, (1 + k) / (10 + k)).  The kernel
        multiplies (p - e) by (float)(1 - d_k)."""
        self._ema_need()
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1")
        return min(self.ema_decay, (1.0 + k) / (10.0 + k)) if self.ema_warmup else self.ema_decay

    @torch.no_grad()
    def _ema_exchange(self):
        """Exchanges the CONTENTS of the parameter arena and the average (the plans are bound to the arena's address), in stream
        order, through one scratch tensor."""
        p, e = self.model.param_arena, self.ema_arena
        tmp = p.detach().clone()
        p.copy_(e)
        e.copy_(tmp)
        del tmp

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model runs on the averaged parameters (with the live BatchNorm statistics): validation, export.
        Every forward packs its weights from the arena anew, so nothing derived goes stale.  A training forward taken on the other
        weights cannot be continued: loss_backward() right behind entry or exit raises.  step(), load_state_dict(), ema_reset() and a
        nested entry raise RuntimeError inside the block; the arenas are exchanged back also when the body raises."""
        self._ema_need()
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is already active")
        self._ema_follow()
        self._ema_exchange()
        self._ema_swapped = True
        self.model._last = None
        try:
            yield self
        finally:
            self._ema_exchange()
            self._ema_swapped = False
            self.model._last = None

    def ema_state_dict(self):
        """The model's state_dict (the reference's layout: keys, order, shapes) with the averaged parameters - clones - and the live
        buffers: the BatchNorm running statistics and num_batches_tracked are not averaged."""
        self._ema_need()
        if self._ema_swapped:
            raise RuntimeError("ema_state_dict() inside ema_weights(): model.state_dict() is the averaged one there")
        self._ema_follow()
        avg, off = {}, 0
        for name, p in self.model.named_parameters():
            n = p.numel()
            avg[name] = self.ema_arena[off:off + n].view(p.shape).clone()
            off += n
        return collections.OrderedDict((k, avg[k] if k in avg else v.detach().clone()) for k, v in self.model.state_dict().items())

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        m = self.model
        if self._ema_swapped:
            raise RuntimeError("step() inside ema_weights(): the parameter arena holds the average")
        if self.exp_avg.device != m.param_arena.device:
            self.exp_avg = self.exp_avg.to(m.param_arena.device)
            self.exp_avg_sq = self.exp_avg_sq.to(m.param_arena.device)
        if self.ema_arena is not None:
            self._ema_follow()
        gd, L = self._guard, _lib.lib()
        if gd is not None and grad_scale != 1.0:
            raise ValueError("grad_scale is not available on the guarded path (the loss scaler divides its scale out itself)")
        n = m.param_arena.numel()
        self._sync_trainable(look=False)
        arenas = (m.param_arena.data_ptr(), m.grad_arena.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n)
        whole = self.ema_arena is None and not self._grouped and self._ranges == [[0, n, 0]]   # (the average always takes the table)
        if whole:
            # Whole arena: no groups, nothing is or ever was frozen - one class, no table.
            g = self.param_groups[0]
            arenas += (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
        else:
            # Table: groups, frozen ranges, step origins - one launch under the segment table, the classes by value.
            classes = self._class_array()
            arenas += (self._ensure_table().data_ptr(), len(self._segments), classes, len(classes))
        if gd is None:
            self.step_count += 1
            if self.ema_arena is not None:
                ema = _lib.AdamEma(self.ema_arena.data_ptr(), self.ema_decay, int(self.ema_warmup), self._ema_k + 1)
                _lib.check(L.dmm_adam_step_segmented_ema(*arenas, self.step_count, float(grad_scale), _lib.stream_ptr(), C.byref(ema)))
                self._ema_k += 1
                return
            step = L.dmm_adam_step if whole else L.dmm_adam_step_segmented
            _lib.check(step(*arenas, self.step_count, float(grad_scale), _lib.stream_ptr()))
            return
        # Guarded: arena reduction(s) -> decision -> Adam, no host synchronisation.  In a data-parallel job call it after
        # GradAllReduce.wait(works): every rank then reads the same summed arena and takes the same decision.
        state = gd._materialize(m.param_arena.device)
        scratch = gd._scratch_for(n)
        tail = (float(self.max_grad_norm or 0.0), gd.growth_factor, gd.backoff_factor, gd.growth_interval, state.data_ptr(), scratch.data_ptr(),
                _lib.stream_ptr())
        if self.ema_arena is not None:   # the device forms k = applied_steps - _ema_t0: a skipped step is no averaging update
            ema = _lib.AdamEma(self.ema_arena.data_ptr(), self.ema_decay, int(self.ema_warmup), self._ema_t0)
            _lib.check(L.dmm_adam_step_guarded_segmented_ema(*arenas, *tail, C.byref(ema)))
            return
        step = L.dmm_adam_step_guarded if whole else L.dmm_adam_step_guarded_segmented
        _lib.check(step(*arenas, *tail))

    # ---- torch.optim.Adam-compatible checkpoint format ----
    def state_dict(self):
        state, off = {}, 0
        self._sync_trainable()
        step_count = self.step_count
        for i, p in enumerate(self.model.parameters()):
            n = p.numel()
            own = self._param_step(i, step_count)   # per parameter, as torch counts; a parameter that never trained has no entry
            if own > 0:
                state[self._torch_index[i]] = {"step": torch.tensor(float(own)),
                            "exp_avg": self.exp_avg[off:off + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[off:off + n].view(p.shape).clone()}
            off += n
        groups = []
        for g in self.param_groups:
            g = dict(g, params=list(g["params"]))
            g.update(maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
            groups.append(g)
        sd = {"state": dict(sorted(state.items())), "param_groups": groups}
        if self._guard is not None:   # torch.optim.Adam.load_state_dict ignores a key it does not know
            sd[_STATE_KEY] = self._guard.state_dict()
        if self.ema_arena is not None:   # (likewise; absent without an average: the key set is then what it always was)
            if self._ema_swapped:
                raise RuntimeError("state_dict() inside ema_weights(): the parameter arena holds the average")
            sd[_EMA_KEY] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "num_updates": self.ema_num_updates,
                            "params": self.ema_arena.detach().cpu().clone()}
        return sd

    def load_state_dict(self, sd):
        if self._ema_swapped:
            raise RuntimeError("load_state_dict() inside ema_weights(): the parameter arena holds the average")
        off = 0
        if self._grouped:   # torch's own check: the same groups, each of the same size
            theirs = sd["param_groups"]
            if len(theirs) != len(self.param_groups):
                raise ValueError(f"loaded state dict has {len(theirs)} parameter groups, the optimiser has {len(self.param_groups)}")
            if any(len(a["params"]) != len(b["params"]) for a, b in zip(theirs, self.param_groups)):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        steps = [int(float(s["step"])) for s in sd["state"].values()] or [0]
        self.step_count = count = max(steps)
        # step origins from the per-parameter steps: a checkpoint written in one phase resumes in that phase.  A trainable parameter
        # without an entry takes its first step next (torch creates its state then); a frozen one without an entry has never trained.
        self._sig = tuple(p.requires_grad for p in self._params)
        self._ranges = None
        for i, p in enumerate(self.model.parameters()):
            n = p.numel()
            s = sd["state"].get(self._torch_index[i])
            own = int(float(s["step"])) if s is not None else 0
            self._t0[i] = count - own if (own > 0 or self._sig[i]) else None
            self._frozen_at[i] = count if (own > 0 and not self._sig[i]) else None
            if s is not None:
                self.exp_avg[off:off + n].copy_(s["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(s["exp_avg_sq"].reshape(-1))
            off += n
        for mine, theirs in zip(self.param_groups, sd["param_groups"]):   # (without groups: the one group there is)
            for k in self._GROUP_KEYS if self._grouped else ("lr", "betas", "eps", "weight_decay"):
                if k in theirs:
                    mine[k] = tuple(theirs[k]) if k == "betas" and self._grouped else theirs[k]
        if self._guard is not None and sd.get(_STATE_KEY) is not None:   # (a checkpoint of the plain path has none: the scaler keeps its state)
            self._guard.load_state_dict(sd[_STATE_KEY])
        # The average: from its key; a checkpoint written without one starts it at the parameters as loaded (the model's state is
        # loaded before the optimiser's).  Decay and warm-up stay the constructor's.  Without an average the key is ignored.
        if self.ema_arena is not None:
            saved = sd.get(_EMA_KEY)
            if saved is None:
                self.ema_reset()
            else:
                params = saved["params"].reshape(-1)
                if params.numel() != self.ema_arena.numel():
                    raise ValueError(f"loaded parameter average has {params.numel()} elements, the arena has {self.ema_arena.numel()}")
                with torch.no_grad():
                    self.ema_arena.copy_(params)
                self._ema_k = int(saved["num_updates"])
                self._ema_t0 = count - self._ema_k if self._guard is not None else 0


def fine_tune_groups(model, lr, weight_decay, encoder_lr_scale=1.0, no_decay_norm_bias=False):
    """Parameter groups of the usual fine-tuning recipe, for ``FusedAdam(model, param_groups=...)`` (or torch.optim.Adam):
    the encoder - what ``model.freeze_encoder()`` freezes: features, stream_2_features, concat_module - at ``encoder_lr_scale * lr``,
    and with ``no_decay_norm_bias`` no weight decay on the BatchNorm weights and biases (the DMM_T_BN_WEIGHT / DMM_T_BN_BIAS tensors
    of the plan's table; the model's convolutions have no bias).  Order: rest, rest without decay, encoder, encoder without decay;
    with ``encoder_lr_scale == 1`` the encoder is part of "rest"; empty groups are left out."""
    if not (math.isfinite(float(encoder_lr_scale)) and float(encoder_lr_scale) >= 0):
        raise ValueError("encoder_lr_scale must be a finite number >= 0")
    enc = {id(p) for p in model._encoder_params} if float(encoder_lr_scale) != 1.0 else set()
    kinds = [kind for _, kind, _, _ in model._table if kind <= _lib.T_BN_BIAS]
    buckets = [[], [], [], []]
    for (_, p), kind in zip(model._named_params, kinds):
        norm = no_decay_norm_bias and kind in (_lib.T_BN_WEIGHT, _lib.T_BN_BIAS)
        buckets[2 * (id(p) in enc) + norm].append(p)
    groups = []
    for k, ps in enumerate(buckets):
        if ps:
            groups.append({"params": ps, "lr": float(lr) * (float(encoder_lr_scale) if k >= 2 else 1.0),
                           "weight_decay": 0.0 if k % 2 else float(weight_decay)})
    return groups
