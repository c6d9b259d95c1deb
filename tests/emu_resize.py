"""EmuPoolBackend plus the entry point of include/sfk_resize.h through tests/ref_resize.py: sfk_u8_pad_resize_cubic."""
import torch

import ref_resize
from emu_pool import EmuPoolBackend


class EmuResizeBackend(EmuPoolBackend):
    def u8_pad_resize_cubic(self, src, offset, hw, out, size, max_side, fill):
        f = offset.shape[0]
        c = out.shape[-1]
        assert src.dtype == torch.uint8 and src.dim() == 1 and offset.dtype == torch.int64 and hw.dtype == torch.int32
        assert tuple(hw.shape) == (f, 2) and out.dtype == torch.uint8 and tuple(out.shape[-3:]) == (size, size, c)
        assert out.numel() == f * size * size * c

        def run(stream):
            got = ref_resize.resize_table(src.numpy(), offset.numpy(), hw.numpy(), c, size, max_side, fill)
            out.copy_(torch.from_numpy(got).reshape(out.shape))
        return run
