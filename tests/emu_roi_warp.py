"""EmuRoiRaggedBackend plus the three entry points of include/sfk_roi_warp.h as calls of tests/ref_roi_warp.py's roi_warp32 --
the contract in float32 torch ops -- on the clips MATERIALISED from the source, so the CPU tests drive the whole pipeline
(RoiResize, FramePool.roi_gather, BoxArena.roi_gather, ResidentGestureSet, prepare_data) through it.  Every launch is noted
in ``log`` by its method name.  mutant: one of ref_roi_warp.MUTANTS, a deliberately wrong kernel the shared checks must refuse:
  'round'    bilinear taps taken at round(src) instead of floor(src)     'blend'    the edge of the resized image blended to zero
  'miss0'    a missing frame sampled as zeros, not lut[fill]             'swap'     the u and v rows of the matrix swapped
  'support'  the antialias support widened by the matrix's own scale     'c_off'    the destination plane offset ignored"""
import torch

from emu_roi_pool import materialise
from emu_roi_ragged import EmuRoiRaggedBackend, materialise_ragged
from ref_roi_warp import roi_warp32

LOGGED = ("roi_resize", "roi_resize_pool", "roi_resize_ragged", "roi_resize_warp", "roi_resize_pool_warp",
          "roi_resize_ragged_warp")


class EmuRoiWarpBackend(EmuRoiRaggedBackend):
    def __init__(self, *a, mutant=None, **kw):
        super().__init__(*a, **kw)
        self.mutant, self.log = mutant, []

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if name in LOGGED:
            log = super().__getattribute__("log")

            def noted(*a, **kw):
                run = attr(*a, **kw)

                def launch(stream):
                    log.append(name)
                    return run(stream)
                return launch
            return noted
        return attr

    def _write(self, out, c_off, c, r):
        out[:, :, 0:c].copy_(r) if self.mutant == "c_off" else out[:, :, c_off:c_off + c].copy_(r)

    def _check(self, n, t, c, box, warp, out, c_off):
        assert box.dtype == torch.int32 and tuple(box.shape) == (n, 4)
        assert warp.dtype == torch.float32 and tuple(warp.shape) == (n, 6)
        assert out.dim() == 5 and out.stride(4) == 1 and tuple(out.shape[:2]) == (n, t) and c_off + c <= out.shape[2]

    def roi_resize_warp(self, src, lut, box, warp, out, antialias, c_off=0):
        n, t, h, w, c = src.shape
        assert src.dtype == torch.uint8
        self._check(n, t, c, box, warp, out, c_off)

        def run(stream):
            self._write(out, c_off, c, roi_warp32(src, lut, box, warp, out.shape[3], out.shape[4], antialias, mutant=self.mutant))
        return run

    def roi_resize_pool_warp(self, pool, index, lut, fill, box, warp, out, antialias, c0=0, c=None, c_off=0):
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and index.dtype == torch.int32 and index.dim() == 2 and 0 <= fill <= 255
        n, t = index.shape
        self._check(n, t, c, box, warp, out, c_off)

        def run(stream):
            miss = (index < 0) | (index >= f)
            r = roi_warp32(materialise(pool, index, fill, c0, c), lut, box, warp, out.shape[3], out.shape[4], antialias, miss.cpu(),
                           fill, self.mutant)
            self._write(out, c_off, c, r)
        return run

    def roi_resize_ragged_warp(self, arena, offset, hw, lut, fill, box, warp, out, antialias, pitch=7, c0=0, c=None, c_off=0,
                               max_hw=None):
        c = pitch - c0 if c is None else c
        n, t = offset.shape
        assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.numel() % 4 == 0 and arena.data_ptr() % 4 == 0
        assert offset.dtype == torch.int64 and hw.dtype == torch.int32 and tuple(hw.shape) == (n, 2) and 0 <= fill <= 255
        self._check(n, t, c, box, warp, out, c_off)
        if max_hw is None:
            max_hw = tuple(max(int(v), 1) for v in hw.max(0).values.tolist())

        def run(stream):
            for i in range(n):
                hn, wn = (int(v) for v in hw[i])
                ok = 1 <= hn <= int(max_hw[0]) and 1 <= wn <= int(max_hw[1])
                miss = torch.tensor([[not (ok and 0 <= int(o) and int(o) + hn * wn * pitch <= arena.numel()) for o in offset[i]]])
                clip = materialise_ragged(arena, offset[i], hw[i], fill, max_hw, pitch, c0, c)
                r = roi_warp32(clip, lut, box[i:i + 1], warp[i:i + 1], out.shape[3], out.shape[4], antialias, miss, fill, self.mutant)
                self._write(out[i:i + 1], c_off, c, r)
        return run
