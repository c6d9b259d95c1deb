"""The exponential moving average of a model's weights (include/sfk_ema.h): which launches keep it and evaluate it.

``WeightEma`` owns no state, as optim.Optimizer owns none: the averaged arena, the averaged BatchNorm running statistics,
the step counter and the uploaded table live on the engine (Engine.optim_state('ema')), one of each per engine.  The eval
plans derive everything from the live arena and the per-layer running statistics at every forward, so "evaluate the
averaged model" is an in-place exchange of contents (sfk_ema_swap) around an ordinary eval forward, with no second set of
plans.  The average and its counter are not checkpointed separately (the optimizer state is not either): a resumed run
starts the average from the loaded weights."""
from __future__ import annotations

import contextlib
from typing import Dict

import torch


class WeightEma:
    def __init__(self, engine, decay: float, warmup: bool = False):
        """decay in [0, 1); warmup: the rate of step t is min(decay, (1 + t) / (10 + t)) (timm's ModelEmaV2)"""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {decay}")
        self.eng, self.decay, self.warmup = engine, decay, bool(warmup)
        engine.optim_state("ema")

    def update_ops(self):
        """sfk_ema_update over the arena and the running statistics: one launch, after the step's last optimizer launch"""
        eng = self.eng
        return eng.be.ema_update(eng.P.data, eng.ema_P, eng.arena_numel, eng.ema_table, self.decay, self.warmup, eng.ema_step)

    def swap_ops(self):
        """sfk_ema_swap: the live model and the average exchange their contents"""
        eng = self.eng
        return eng.be.ema_swap(eng.P.data, eng.ema_P, eng.arena_numel, eng.ema_table)

    @contextlib.contextmanager
    def applied(self):
        """inside, the engine holds the averaged weights and statistics (and the average the live ones); on exit they are
        swapped back, so the live model has its earlier bits.  Both swaps run on the current stream."""
        swap = self.swap_ops()
        swap(self.eng._stream())
        try:
            yield self
        finally:
            swap(self.eng._stream())

    def reset(self):
        """the average becomes a copy of the live model again and the counter zero (after a checkpoint load)"""
        eng = self.eng
        with torch.no_grad():
            eng.ema_P.copy_(eng.P.data)
            for live, avg in eng.ema_stat_pairs():
                avg.copy_(live)
            eng.ema_step.zero_()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """the engine's state_dict() of the averaged model; num_batches_tracked and the dead tensors are the live model's"""
        with self.applied():
            return self.eng.state_dict()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """loads a flat state_dict into the AVERAGE; the live model keeps its weights, statistics and counters"""
        eng = self.eng
        keep = ([L.nbt.clone() for L in eng.layers], {k: v.clone() for k, v in eng.dead.items()})
        with self.applied():
            try:
                return eng.load_state_dict(sd, strict)
            finally:
                for L, n in zip(eng.layers, keep[0]):
                    L.nbt.copy_(n)
                eng.dead = keep[1]
