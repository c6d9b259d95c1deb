"""EmuOptimBackend plus the entry points of include/sfk_groups.h, stated as their contract: sfk_adam_groups / sfk_sgd_groups
loop over the segments and call the parent's adam_hp / sgd_hp on each slice with a cloned step counter, the group's rate row
and weight decay and decay_count = decay ? e - b : 0; sfk_grad_norm_groups is the parent's grad_norm on a copy with the
uncovered elements zeroed.  The class attributes switch on the mutations tests/test_groups_cpu.py must see rejected."""
import numpy as np
import torch

from emu_optim import DECAY_MODES, EmuOptimBackend

MAX_SEGS, MAX_GROUPS = 2048, 64          # include/sfk_groups.h SFK_GROUPS_MAX_*


class EmuGroupTable:
    def __init__(self, segments, wds, count):
        self.segments, self.wds, self.count, self.ngroups = segments, wds, count, len(wds)

    @property
    def nsegs(self):
        return len(self.segments)


def check_segments(segments, count, ngroups):
    """the host-side rejections of include/sfk_groups.h"""
    if len(segments) > MAX_SEGS or not 1 <= ngroups <= MAX_GROUPS or count <= 0:
        raise ValueError("sfk_groups: invalid argument")
    prev = 0
    for b, e, grp, _ in segments:
        if b < prev or b >= e or e > count or not 0 <= grp < ngroups:
            raise ValueError("sfk_groups: invalid argument")
        prev = e


class EmuGroupsBackend(EmuOptimBackend):
    visit_frozen = False         # the elements no segment covers are updated too (as group 0, no decay)
    skip_segment_last = False    # a segment's last element is not visited
    wrong_group_row = False      # group j reads the rate row and the decay of group j + 1
    ignore_decay_flag = False    # every covered element decays
    norm_over_frozen = False     # the norm is taken over the whole arena

    def group_table(self, segments, weight_decays, count, device=None):
        segments = [tuple(int(x) for x in s) for s in segments]
        check_segments(segments, count, len(weight_decays))
        return EmuGroupTable(segments, [float(np.float32(w)) for w in weight_decays], count)

    def _walk(self, table):
        segs = []
        prev = 0
        for b, e, grp, dec in table.segments:
            if self.visit_frozen and b > prev:
                segs.append((prev, b, 0, 0))
            prev = e
            if self.skip_segment_last:
                e -= 1
            if self.wrong_group_row:
                grp = (grp + 1) % table.ngroups
            if self.ignore_decay_flag:
                dec = 1
            if e > b:
                segs.append((b, e, grp, dec))
        if self.visit_frozen and prev < table.count:
            segs.append((prev, table.count, 0, 0))
        return segs

    @staticmethod
    def _check_launch(table, count, lr_rows, decay_mode, max_mode):
        mode = DECAY_MODES[decay_mode] if isinstance(decay_mode, str) else int(decay_mode)
        if (table.count != count or lr_rows is None or lr_rows.dim() != 2 or lr_rows.shape[0] != table.ngroups
                or lr_rows.shape[1] <= 0 or not 0 <= mode <= max_mode):
            raise ValueError("sfk_groups_hp: invalid argument")
        check_segments(table.segments, count, table.ngroups)
        return mode

    def adam_groups(self, p, g, m, v, count, table, lr_rows, b1, b2, eps, gscale, step, shadow=None, decay_mode="none",
                    clip_coef=None):
        mode = self._check_launch(table, count, lr_rows, decay_mode, 2)

        def run(stream):
            for b, e, grp, dec in self._walk(table):
                st = step.clone()
                EmuOptimBackend.adam_hp(self, p[b:e], g[b:e], m[b:e], v[b:e], e - b, lr_rows[grp], b1, b2, eps, gscale, st,
                                        None if shadow is None else shadow[b:e], weight_decay=table.wds[grp], decay_mode=mode,
                                        decay_count=e - b if dec else 0, clip_coef=clip_coef)(stream)
            step.add_(1)
        return run

    def sgd_groups(self, p, g, buf, count, table, lr_rows, momentum, dampening, nesterov, gscale, step, shadow=None,
                   decay_mode="none", clip_coef=None):
        mode = self._check_launch(table, count, lr_rows, decay_mode, 1)

        def run(stream):
            for b, e, grp, dec in self._walk(table):
                st = step.clone()
                EmuOptimBackend.sgd_hp(self, p[b:e], g[b:e], None if buf is None else buf[b:e], e - b, lr_rows[grp], momentum,
                                       dampening, nesterov, gscale, st, None if shadow is None else shadow[b:e],
                                       weight_decay=table.wds[grp], decay_mode=mode, decay_count=e - b if dec else 0,
                                       clip_coef=clip_coef)(stream)
            step.add_(1)
        return run

    def grad_norm_groups(self, g, count, table, gscale, max_norm, partials, out):
        check_segments(table.segments, count, table.ngroups)
        if table.count != count:
            raise ValueError("sfk_grad_norm_groups: invalid argument")

        def run(stream):
            z = g[:count].clone()
            if not self.norm_over_frozen:
                keep = torch.zeros(count, dtype=torch.bool, device=g.device)
                for b, e, _, _ in table.segments:
                    keep[b:e] = True
                z = torch.where(keep, z, torch.zeros_like(z))        # (a NaN in a frozen range does not show)
            EmuOptimBackend.grad_norm(self, z, count, gscale, max_norm, partials, out)(stream)
        return run
