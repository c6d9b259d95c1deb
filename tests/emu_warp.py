"""EmuResidentBackend plus the entry point of include/sfk_warp.h as a call of tests/ref_warp.py's warp32 -- the contract in
float32 torch ops -- so the CPU tests drive the whole pipeline (DevicePreprocess, FramePool.gather, ResidentTrainSet,
prepare_data) through it.  mutant: one of ref_warp.MUTANTS, a deliberately wrong kernel that the shared checks must refuse:
  'round'  taps taken at round(xs) instead of floor(xs)        'clamp'  out-of-frame taps clamped to the edge instead of zero
  'miss0'  a missing frame sampled as zeros, not lut[fill]     'swap'   the x and y rows of the matrix swapped
  'c0'     the channel offset c0 ignored"""
import torch

from emu_resident import EmuResidentBackend
from ref_warp import warp32


class EmuWarpBackend(EmuResidentBackend):
    def __init__(self, *a, mutant=None, **kw):
        super().__init__(*a, **kw)
        self.mutant = mutant

    def u8_pool_gather_warp(self, pool, index, lut, fill, warp, out, c0=0, c=None):
        if index is None:
            assert pool.dim() == 5, "index=None: pool is the stacked (N,T,H,W,P) batch"
            n, t, h, w, p = pool.shape
        else:
            assert pool.dim() == 4 and index.dtype == torch.int32 and index.dim() == 2
            (_, h, w, p), (n, t) = pool.shape, index.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and tuple(out.shape) == (n, t, c, h, w), (tuple(out.shape), (n, t, c, h, w))
        assert warp.dtype == torch.float32 and tuple(warp.shape) == (n, 6) and 0 <= fill <= 255

        def run(stream):
            out.copy_(warp32(pool, index, lut, fill, warp, c0, c, mutant=self.mutant))
        return run

    def warp_fallback_tiles(self, h, w, pixel_pitch, c, row):
        raise NotImplementedError("the emulation has no tiles: sfk_warp_fallback_tiles is the built library's")
