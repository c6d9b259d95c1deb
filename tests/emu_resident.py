"""EmuResizeBackend plus the entry point of include/sfk_resident.h as plain torch indexing: sfk_u8_pool_gather_crop."""
import torch

from emu_pool import pool_gather_crop  # noqa: F401  (re-exported: the tests import it from here)
from emu_resize import EmuResizeBackend


class EmuResidentBackend(EmuResizeBackend):
    def u8_pool_gather_crop(self, pool, index, lut, fill, crop, pad, out, c0=0, c=None):
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and index.dtype == torch.int32 and tuple(out.shape) == tuple(index.shape) + (c, h, w)
        assert crop is None or (crop.dtype == torch.int32 and tuple(crop.shape) == (index.shape[0], 2))
        assert pad >= 0

        def run(stream):
            out.copy_(pool_gather_crop(pool, index, lut, fill, crop, pad, c0, c))
        return run
