"""The optimizer of a TrainStep: which launch an optimizer step is, and over which slice of the arenas.

``Optimizer`` validates the optimizer keywords once, decides the route -- `hp` False: sfk_adam / sfk_sgd with `lr` by value;
True: sfk_adam_hp / sfk_sgd_hp (include/sfk_optim.h) with the rate of step s read from a device table, weight decay and
clipping; `grouped` (implies hp): sfk_adam_groups / sfk_sgd_groups (include/sfk_groups.h) over the arena segments of the
parameter groups, one rate row and one decay per group, frozen ranges in no segment -- and builds the launches.  It owns no state: the moments, the momentum buffer, the step counters and the norm live
on the engine under their names (Engine.optim_state), one tensor per engine whatever number of TrainSteps share it, and are
allocated when a launch that needs them is first built."""
from __future__ import annotations

import math
from functools import partial

import torch


class Optimizer:
    def __init__(self, engine, optimizer: str = "adam", lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False, lr_table=None,
                 weight_decay: float = 0.0, decay_mode: str = "none", decay_scope: str = "weights",
                 clip_grad_norm: float = 0.0, param_groups=(), freeze=()):
        """param_groups: (selector, lr_mult) or (selector, lr_mult, wd_mult) in priority order, freeze: selectors
        (Engine._matcher's: state_dict() key prefixes, '@fresh', '@pretrained'; the first match wins, freeze beats groups)."""
        if optimizer not in ("adam", "sgd"):
            raise ValueError(f"optimizer={optimizer!r}: 'adam' or 'sgd'")
        if decay_mode not in ("none", "l2", "decoupled"):
            raise ValueError(f"decay_mode={decay_mode!r}: 'none', 'l2' or 'decoupled'")
        if decay_scope not in ("weights", "all"):
            raise ValueError(f"decay_scope={decay_scope!r}: 'weights' or 'all'")
        if weight_decay < 0 or clip_grad_norm < 0:
            raise ValueError("weight_decay and clip_grad_norm must not be negative")
        if weight_decay == 0 or decay_mode == "none":
            weight_decay, decay_mode = 0.0, "none"
        if optimizer == "sgd" and decay_mode == "decoupled":
            raise ValueError("decay_mode='decoupled' needs optimizer='adam': torch has no decoupled SGD")
        self.eng, self.optimizer, self.lr, self.betas, self.eps = engine, optimizer, lr, betas, eps
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov
        self.weight_decay, self.decay_mode, self.decay_scope = float(weight_decay), decay_mode, decay_scope
        self.clip_grad_norm = float(clip_grad_norm)
        groups, self.freeze = self._check_groups(param_groups), tuple(freeze)
        self.grouped = bool(groups) or bool(self.freeze)  # the sfk_groups.h route
        self.hp = (lr_table is not None or decay_mode != "none" or self.clip_grad_norm > 0     # the sfk_optim.h route
                   or self.grouped)
        self.lr_table = None                              # device float32: the hp launches index it with their step counter
        if self.hp:
            t = torch.as_tensor([lr] if lr_table is None else lr_table, dtype=torch.float32).reshape(-1)
            if t.numel() < 1:
                raise ValueError("lr_table: at least one rate")
            self.lr_table = t.to(engine.device).contiguous()
        self.segments = self.lr_rows = self.group_decays = None
        self._tables = {}                                 # (lo, hi) -> the backend's group table of the segments inside it
        if self.grouped:
            # the tables of the grouped route, once: the segments, row j = f32(float64(rate_k) * lr_mult_j) of the Python-float
            # table (row 0, multiplier 1, is lr_table bit for bit), decay j = f32(weight_decay * wd_mult_j)
            self.segments = engine.param_segments([g[0] for g in groups], self.freeze, decay_scope)
            if not self.segments:
                raise ValueError(f"freeze={list(self.freeze)!r} leaves nothing trainable")
            if len(self.segments) > self.MAX_SEGS:
                raise ValueError(f"param_groups / freeze cut the arena into {len(self.segments)} segments: at most {self.MAX_SEGS}")
            mults = torch.tensor([1.0] + [g[1] for g in groups], dtype=torch.float64)
            src = torch.as_tensor([lr] if lr_table is None else lr_table, dtype=torch.float64).reshape(1, -1)
            self.lr_rows = (src * mults.reshape(-1, 1)).to(torch.float32).to(engine.device).contiguous()
            self.group_decays = [self.weight_decay * m for m in [1.0] + [g[2] for g in groups]]
        self.grad_norm = None                             # engine.grad_norm once a clipped step has been built
        # two launches beside the step's last kernel: Adam only (sfk_sgd is one launch, always), and never with clipping --
        # the coefficient needs the last filter gradient, which the main launch does not wait for
        self.can_split = optimizer == "adam" and not self.clip_grad_norm > 0

    MAX_SEGS, MAX_GROUPS = 2048, 64                       # include/sfk_groups.h SFK_GROUPS_MAX_*

    @classmethod
    def _check_groups(cls, param_groups):
        """[(selector, lr_mult, wd_mult)] of the `param_groups` keyword"""
        out = []
        for g in param_groups:
            if isinstance(g, str) or not hasattr(g, "__len__") or len(g) not in (2, 3):
                raise ValueError(f"param_groups entry {g!r}: (selector, lr_mult) or (selector, lr_mult, wd_mult)")
            sel, mults = g[0], [float(x) for x in g[1:]] + [1.0] * (3 - len(g))
            for name, x in zip(("lr_mult", "wd_mult"), mults):
                if not math.isfinite(x) or x < 0:
                    raise ValueError(f"param_groups entry {tuple(g)!r}: {name}={x} must be finite and not negative")
            out.append((sel, mults[0], mults[1]))
        if len(out) > cls.MAX_GROUPS - 1:
            raise ValueError(f"param_groups: {len(out)} selectors, at most {cls.MAX_GROUPS - 1} ({cls.MAX_GROUPS} groups with "
                             "the unmatched rest)")
        return out

    def _group_table(self, lo: int, hi: int):
        """the segments inside [lo, hi), relative to lo, as the backend's table (built once per slice)"""
        t = self._tables.get((lo, hi))
        if t is None:
            segs = [(max(b, lo) - lo, min(e, hi) - lo, grp, dec) for b, e, grp, dec in self.segments if b < hi and e > lo]
            t = self._tables[(lo, hi)] = self.eng.be.group_table(segs, self.group_decays, hi - lo, self.eng.device)
        return t

    def _counter(self):
        """the step counter the whole-arena launch keeps on the device (None before the first build)"""
        return self.eng.sgd_step if self.optimizer == "sgd" else self.eng.adam_step

    def _launch(self, lo: int, hi: int, step, grad_scale: float, clip_coef):
        """one optimizer launch over arena elements [lo, hi) with the counter `step` (the launch increments it).  The only
        place that slices the arenas, makes decay_count (grouped: the segments) relative to the slice and picks the backend
        call."""
        eng, be, sgd = self.eng, self.eng.be, self.optimizer == "sgd"
        state = (eng.sgd_buf,) if sgd else (eng.adam_m, eng.adam_v)
        hyper = (self.momentum, self.dampening, self.nesterov) if sgd else (self.betas[0], self.betas[1], self.eps)
        arenas = [t[lo:hi] for t in (eng.P.data, eng.G) + state]
        if not self.hp:
            return (be.sgd if sgd else be.adam)(*arenas, hi - lo, self.lr, *hyper, grad_scale, step, None)
        if self.grouped:                                  # per segment, its decay flag stands where decay_count does below
            return (be.sgd_groups if sgd else be.adam_groups)(*arenas, hi - lo, self._group_table(lo, hi), self.lr_rows, *hyper,
                                                              grad_scale, step, None, decay_mode=self.decay_mode,
                                                              clip_coef=clip_coef)
        dc = eng.decay_count(self.decay_scope)            # arena elements [0, dc) decay
        return (be.sgd_hp if sgd else be.adam_hp)(*arenas, hi - lo, self.lr_table, *hyper, grad_scale, step, None,
                                                  weight_decay=self.weight_decay, decay_mode=self.decay_mode,
                                                  decay_count=min(max(dc - lo, 0), hi - lo), clip_coef=clip_coef)

    def norm_ops(self, grad_scale: float = 1.0):
        """sfk_grad_norm over the whole gradient arena, to run after the finished (reduced) backward: engine.grad_norm =
        (||G * grad_scale||_2, min(1, max_norm / (norm + 1e-6))), float32[2] on the device.  None without clipping.  Grouped:
        sfk_grad_norm_groups with the whole table -- frozen gradients, a NaN among them included, do not show."""
        if not self.clip_grad_norm > 0:
            return None
        eng = self.eng
        eng.optim_state("grad_norm")
        self.grad_norm = eng.grad_norm
        if self.grouped:
            return eng.be.grad_norm_groups(eng.G, eng.arena_numel, self._group_table(0, eng.arena_numel), grad_scale,
                                           self.clip_grad_norm, eng.grad_norm_parts, eng.grad_norm)
        return eng.be.grad_norm(eng.G, eng.arena_numel, grad_scale, self.clip_grad_norm, eng.grad_norm_parts, eng.grad_norm)

    def update_ops(self, grad_scale: float = 1.0):
        """the update over the whole arena in one launch; with clipping it reads the coefficient norm_ops leaves"""
        eng = self.eng
        eng.optim_state(self.optimizer)
        coef = None
        if self.clip_grad_norm > 0:
            eng.optim_state("grad_norm")
            coef = eng.grad_norm[1:2]
        return self._launch(0, eng.arena_numel, self._counter(), grad_scale, coef)

    def split_ops(self, cut: int, grad_scale: float = 1.0):
        """(main, tail, set_tail): the same update in two launches -- [cut, n) with the step counter and [0, cut) with the
        tail counter, element-wise identical to the single launch.  Every launch increments the counter it is given, so
        set_tail() (tail counter = step - 1) goes between main and tail; where is the caller's choice.  TrainStep never
        splits a segmented step, so the reducer's world is 1 there and the grad_scale it passes is 1."""
        assert self.can_split
        eng = self.eng
        eng.optim_state("adam")
        main = self._launch(cut, eng.arena_numel, eng.adam_step, grad_scale, None)
        tail = self._launch(0, cut, eng.adam_step_tail, grad_scale, None)
        return main, tail, partial(torch.sub, eng.adam_step, 1, out=eng.adam_step_tail)

    def _last_index(self) -> int:
        step = self._counter()
        s = int(step[0]) if step is not None else 0
        return min(max(s, 1), self.lr_table.numel()) - 1

    def last_lr(self) -> float:
        """the rate the last optimizer step used (one device read: the step counter); grouped: group 0's"""
        if not self.hp:
            return float(self.lr)
        return float(self.lr_table[self._last_index()])

    def last_lrs(self) -> list:
        """one rate per group, group 0 (the unmatched rest) first; a single rate without groups"""
        if not self.grouped:
            return [self.last_lr()]
        return [float(x) for x in self.lr_rows[:, self._last_index()]]
