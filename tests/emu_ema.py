"""EmuMixBackend plus the two entry points of include/sfk_ema.h as torch ops, both stated through tests/ref_ema.py, with the
host-side rejections of the header.  `launches` also notes every EMA launch that RAN.  The class attributes switch on the
mutations tests/test_ema_cpu.py must see rejected."""
import torch

from emu_mix import EmuMixBackend
from ref_ema import ema_weight, ref_ema

EMA_MAX_TENSORS = 4096       # include/sfk_ema.h SFK_EMA_MAX_TENSORS


class EmuEmaTable:
    def __init__(self, pairs):
        self.pairs = pairs

    @property
    def ntensors(self) -> int:
        return len(self.pairs)


class EmuEmaBackend(EmuMixBackend):
    warmup_ignored = False       # d_t = decay whatever the flag says
    step_before_increment = False    # t - 1 instead of t
    table_skipped = False        # the table tensors are left as they are
    last_element_skipped = False     # the arena's last element is not visited
    swap_copies = False          # e = p instead of an exchange
    convex_form = False          # d * e + w * p instead of e + w * (p - e)

    def ema_table(self, pairs):
        pairs = [(s, d) for s, d in pairs]
        if len(pairs) > EMA_MAX_TENSORS:
            raise ValueError("sfk_ema table: too many tensors")
        for s, d in pairs:
            if s.dtype != torch.float32 or d.dtype != torch.float32 or s.numel() != d.numel() or s.numel() < 1:
                raise ValueError("sfk_ema table entry: two float32 tensors of the same size")
        return EmuEmaTable(pairs)

    @staticmethod
    def _check(p, e, count, table):
        if p is None or e is None or count <= 0 or (table is not None and table.ntensors > EMA_MAX_TENSORS):
            raise ValueError("sfk_ema_desc: invalid argument")

    def _one(self, e, p, w, d):
        if self.convex_form:
            return torch.tensor(d, dtype=torch.float32) * e + torch.tensor(w, dtype=torch.float32) * p
        return ref_ema(e, p, w)

    def ema_update(self, p, e, count, table, decay, warmup, step):
        self._check(p, e, count, table)
        if step is None or not 0.0 <= decay < 1.0:
            raise ValueError("sfk_ema_update: invalid argument")

        def run(stream):
            self.launches.append("ema_update")
            step.add_(1)
            t = int(step[0]) - (1 if self.step_before_increment else 0)
            w = ema_weight(decay, warmup and not self.warmup_ignored, t)
            n = count - 1 if self.last_element_skipped else count
            e[:n] = self._one(e[:n], p[:n], w, 1.0 - w)
            if table is not None and not self.table_skipped:
                for s, d in table.pairs:
                    d.copy_(self._one(d, s, w, 1.0 - w))
        return run

    def ema_swap(self, p, e, count, table):
        self._check(p, e, count, table)

        def run(stream):
            self.launches.append("ema_swap")
            pairs = [(p[:count], e[:count])] + (list(table.pairs) if table is not None else [])
            for a, b in pairs:
                if self.swap_copies:
                    b.copy_(a)
                    continue
                ai, bi = a.view(torch.int32), b.view(torch.int32)
                keep = ai.clone()
                ai.copy_(bi)
                bi.copy_(keep)
        return run
