"""EmuAugBackend plus the entry point of include/sfk_pool.h as plain torch indexing: sfk_u8_pool_gather -- the formula of
include/sfk_resident.h (``pool_gather_crop``, which emu_resident.py shares) without a crop."""
import torch

from emu_aug import EmuAugBackend


def pool_gather_crop(pool, index, lut, fill, crop, pad, c0, c):
    """the header's formula, element by element in torch, for ANY crop and index values: (n, t, c, h, w) float32"""
    f, h, w, p = pool.shape
    n, t = index.shape
    idx = index.long()
    miss = (idx < 0) | (idx >= f)
    x = lut[pool[idx.clamp(0, f - 1)][..., c0:c0 + c].long()]                    # (n, t, h, w, c) fp32
    x = torch.where(miss[:, :, None, None, None], lut[fill], x)
    if crop is None:
        return x.permute(0, 1, 4, 2, 3).contiguous()
    out = torch.zeros(n, t, c, h, w, dtype=torch.float32)
    for i in range(n):
        ys = torch.arange(h) + int(crop[i, 0]) - pad
        xs = torch.arange(w) + int(crop[i, 1]) - pad
        inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
        g = x[i][:, ys.clamp(0, h - 1)][:, :, xs.clamp(0, w - 1)]                # (t, h, w, c)
        out[i] = torch.where(inside[None, :, :, None], g, torch.zeros(())).permute(0, 3, 1, 2)
    return out


class EmuPoolBackend(EmuAugBackend):
    def u8_pool_gather(self, pool, index, lut, fill, out, c0=0, c=None):
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and index.dtype == torch.int32 and tuple(out.shape) == tuple(index.shape) + (c, h, w)

        def run(stream):
            out.copy_(pool_gather_crop(pool, index, lut, fill, None, 0, c0, c))
        return run
