"""EmuAugBackend plus the four entry points of include/sfk_optim.h as torch ops in honest float32: every product, sum,
quotient and root is one float32 torch op (nothing fused), the hyper-parameters are the float32 values the C ABI carries, the
bias corrections and 1 - lr*wd are formed in double and rounded, the step is read after its increment.  The class
attributes switch on the mutations tests/test_optim_cpu.py must see rejected."""
import numpy as np
import torch

from emu_aug import EmuAugBackend

DECAY_MODES = {"none": 0, "l2": 1, "decoupled": 2}
NORM_ROW_ELEMS, NORM_MAX_PARTS = 4096, 2048        # csrc/optim_sched.hip, include/sfk_optim.h


def _f(x) -> float:
    return float(np.float32(x))


class EmuOptimBackend(EmuAugBackend):
    decay_after_update = False   # the decay applied to the updated parameters
    decay_wrong_range = False    # [decay_count, count) decays instead of [0, decay_count)
    coef_unclamped = False       # out[1] = max_norm / (norm + 1e-6), above 1 too
    table_off = 0                # 1: lr_table[s] instead of lr_table[s - 1]
    table_unclamped = False      # no clamp at lr_len (the index wraps instead of reading past the table)
    norm_before_scale = False    # ||g|| instead of ||g * grad_scale||
    skip_mod4_tail = False       # the last count % 4 elements are not visited
    grid_cap = None              # elements beyond it are not visited

    def _visited(self, count: int) -> int:
        n = count - count % 4 if self.skip_mod4_tail else count
        return n if self.grid_cap is None else min(n, self.grid_cap)

    def _lr(self, lr_table, s: int) -> float:
        n = lr_table.numel()
        i = max(s, 1) + self.table_off
        i = (i - 1) % n + 1 if self.table_unclamped else min(i, n)
        return float(lr_table[i - 1])

    def _decay_slice(self, count: int, decay_count: int) -> slice:
        return slice(decay_count, count) if self.decay_wrong_range else slice(0, decay_count)

    @staticmethod
    def _check_hp(count, lr_table, decay_mode, decay_count, max_mode):
        mode = DECAY_MODES[decay_mode] if isinstance(decay_mode, str) else int(decay_mode)
        if lr_table is None or lr_table.numel() <= 0 or not 0 <= mode <= max_mode or not 0 <= decay_count <= count:
            raise ValueError("sfk_optim_hp: invalid argument")
        return mode

    def _grad(self, g, p, n, gscale, clip_coef, l2, wd, ds):
        gs = g[:n] * _f(gscale)
        if clip_coef is not None:
            gs = gs * float(clip_coef[0])
        if l2 and not self.decay_after_update:
            d = slice(ds.start, min(ds.stop, n))
            gs[d] = gs[d] + _f(wd) * p[:n][d]
        return gs

    def adam_hp(self, p, g, m, v, count, lr_table, b1, b2, eps, gscale, step, shadow=None, weight_decay: float = 0.0,
                decay_mode="none", decay_count: int = 0, clip_coef=None):
        mode = self._check_hp(count, lr_table, decay_mode, decay_count, 2)

        def run(stream):
            step.add_(1)
            s = int(step[0])
            f = np.float32
            lr = self._lr(lr_table, s)
            n = self._visited(count)
            ds = self._decay_slice(count, decay_count)
            d = slice(ds.start, min(ds.stop, n))
            b1_, b2_ = f(b1), f(b2)
            bc1, bc2 = f(1.0 - float(b1_) ** s), f(1.0 - float(b2_) ** s)
            neg_step, inv_sqrt_bc2 = float(-(f(lr) / bc1)), float(f(1.0) / np.sqrt(bc2))
            mul = _f(1.0 - lr * _f(weight_decay))
            gs = self._grad(g, p, n, gscale, clip_coef, mode == 1, weight_decay, ds)
            p0 = p[:n].clone()
            if mode == 2 and not self.decay_after_update:
                p0[d] = p0[d] * mul
            m1 = float(b1_) * m[:n] + float(f(1.0) - b1_) * gs
            v1 = float(b2_) * v[:n] + (float(f(1.0) - b2_) * gs) * gs
            den = v1.sqrt() * inv_sqrt_bc2 + _f(eps)
            p1 = p0 + neg_step * (m1 / den)
            if self.decay_after_update and mode == 2:
                p1[d] = p1[d] * mul
            if self.decay_after_update and mode == 1:
                p1[d] = p1[d] - (lr * _f(weight_decay)) * p1[d]
            m[:n], v[:n], p[:n] = m1, v1, p1
            if shadow is not None:
                shadow[:n].copy_(p[:n])
        return run

    def sgd_hp(self, p, g, buf, count, lr_table, momentum, dampening, nesterov, gscale, step, shadow=None,
               weight_decay: float = 0.0, decay_mode="none", decay_count: int = 0, clip_coef=None):
        mode = self._check_hp(count, lr_table, decay_mode, decay_count, 1)

        def run(stream):
            step.add_(1)
            s = int(step[0])
            lr = self._lr(lr_table, s)
            n = self._visited(count)
            ds = self._decay_slice(count, decay_count)
            gs = self._grad(g, p, n, gscale, clip_coef, mode == 1, weight_decay, ds)
            dd = gs
            if momentum != 0:
                b = gs.clone() if s == 1 else _f(momentum) * buf[:n] + _f(1.0 - _f(dampening)) * gs
                buf[:n] = b
                dd = gs + _f(momentum) * b if nesterov else b
            p1 = p[:n] + (-lr) * dd
            if self.decay_after_update and mode == 1:
                d = slice(ds.start, min(ds.stop, n))
                p1[d] = p1[d] - (lr * _f(weight_decay)) * p1[d]
            p[:n] = p1
            if shadow is not None:
                shadow[:n].copy_(p[:n])
        return run

    def grad_norm_parts(self, count: int) -> int:
        if count <= 0:
            raise ValueError("sfk_grad_norm_parts: invalid argument")
        return max(1, min(NORM_MAX_PARTS, (count + NORM_ROW_ELEMS - 1) // NORM_ROW_ELEMS))

    def grad_norm(self, g, count, gscale, max_norm, partials, out):
        assert partials.dtype == torch.float64 and partials.numel() >= self.grad_norm_parts(count)

        def run(stream):
            n = self._visited(count)
            x = g[:n] if self.norm_before_scale else g[:n] * _f(gscale)
            norm = (x.double() * x.double()).sum().sqrt().to(torch.float32)
            c = _f(max_norm) / (norm + _f(1e-6))
            out[0] = norm
            out[1] = c if self.coef_unclamped else torch.where(c > 1.0, torch.ones_like(c), c)
        return run
