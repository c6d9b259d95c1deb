"""EmuU8StemPoolBackend plus the entry points of include/sfk_mix.h as torch ops, both stated through tests/ref_mix.py:
sfk_clip_mix as ref_mix written back in place, sfk_softmax_ce_mix as the float64 restatement rounded to float32.  The
backend also notes, in `launches`, every loss and mix launch that RAN (the trainer tests read it)."""
import torch

from emu_u8stem_pool import EmuU8StemPoolBackend
from ref_mix import ref_mix, ref_softmax_ce_mix


class EmuMixBackend(EmuU8StemPoolBackend):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.launches = []

    def softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct):
        run = super().softmax_ce(logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct)

        def noted(stream):
            self.launches.append("softmax_ce")
            return run(stream)
        return noted

    def clip_mix(self, clip, rows, c_off: int = 0, c=None):
        assert clip.dim() == 5 and clip.stride(4) == 1
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (clip.shape[0], 8)

        def run(stream):
            self.launches.append("clip_mix")
            clip.copy_(self._mixed(clip, rows, c_off, c))
        return run

    def _mixed(self, clip, rows, c_off, c):
        return ref_mix(clip, rows, c_off, c)

    def softmax_ce_mix(self, logits, labels, rows, smoothing, n, k, gscale, dlogits, loss_out, loss_sum, correct):
        assert rows is None or (rows.dtype == torch.float32 and tuple(rows.shape) == (n, 8))
        assert 0.0 <= smoothing < 1.0

        def run(stream):
            self.launches.append("softmax_ce_mix")
            own = rows is None or bool(((rows[:, 0] == torch.arange(n, device=rows.device)) & (rows[:, 6] == 1)).all())
            if smoothing == 0 and own:              # the header: then dlogits and correct carry sfk_softmax_ce's bits
                return EmuU8StemPoolBackend.softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum,
                                                       correct)(stream)
            ref =self._loss(logits.reshape(-1)[: n * k].view(n, k), labels[:n], rows, smoothing, gscale)
            if dlogits is not None:
                dlogits.reshape(-1)[: n * k].copy_(ref["dl"].to(torch.float32).reshape(-1))
            if loss_out is not None:
                loss_out[0] += float(ref["loss"])
            if loss_sum is not None:
                loss_sum[0] += float(ref["loss"])
            if correct is not None:
                correct[0] += ref["correct"]
        return run

    def _loss(self, lg, labels, rows, smoothing, gscale):
        return ref_softmax_ce_mix(lg, labels, rows, smoothing, gscale)
