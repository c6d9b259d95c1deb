"""EmuAugBackend plus the entry point of include/sfk_pool.h as plain torch indexing: sfk_u8_pool_gather."""
import torch

from emu_aug import EmuAugBackend


class EmuPoolBackend(EmuAugBackend):
    def u8_pool_gather(self, pool, index, lut, fill, out, c0=0, c=None):
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and index.dtype == torch.int32 and tuple(out.shape) == tuple(index.shape) + (c, h, w)

        def run(stream):
            idx = index.long()
            miss = (idx < 0) | (idx >= f)
            x = lut[pool[idx.clamp(0, f - 1)][..., c0:c0 + c].long()]            # (n, t, h, w, c) fp32
            x = torch.where(miss[:, :, None, None, None], lut[fill], x)
            out.copy_(x.permute(0, 1, 4, 2, 3))
        return run
