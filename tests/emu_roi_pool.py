"""EmuResidentBackend plus the entry point of include/sfk_roi_pool.h as torch ops: sfk_roi_resize_pool is ``roi_resize_ref``
(tests/emu_v2.py) on the clips MATERIALISED from the pool -- the header's own statement of the contract."""
import torch

from emu_resident import EmuResidentBackend
from emu_v2 import roi_resize_ref


def materialise(pool, index, fill: int, c0: int = 0, c=None):
    """(N, T, H, W, c) uint8: frame index[n, t] of the pool, channels c0 .. c0+c-1; bytes of fill for an index outside it"""
    f = pool.shape[0]
    c = pool.shape[3] - c0 if c is None else c
    i = index.long()
    ext = torch.cat([pool, torch.full_like(pool[:1], fill)])
    return ext[torch.where((i < 0) | (i >= f), torch.tensor(f, device=i.device), i)][..., c0:c0 + c]


class EmuRoiPoolBackend(EmuResidentBackend):
    def roi_resize_pool(self, pool, index, lut, fill, box, out, antialias, crop=None, pad=0, c0=0, c=None, c_off=0):
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and index.dtype == torch.int32 and box.dtype == torch.int32
        assert tuple(box.shape) == (index.shape[0], 4) and tuple(out.shape[:2]) == tuple(index.shape) and c_off + c <= out.shape[2]
        assert crop is None or (crop.dtype == torch.int32 and tuple(crop.shape) == (index.shape[0], 2))

        def run(stream):
            r = roi_resize_ref(materialise(pool, index, fill, c0, c), lut, box, out.shape[3], out.shape[4], antialias, crop, pad)
            out[:, :, c_off:c_off + c].copy_(r)
        return run
