"""EmuRoiRaggedBackend plus the four entry points of include/sfk_u8stem_pool.h (the uint8 stems reading the frame pool through
its index table) as torch ops: the virtual clip is materialised with the header's formula -- ``pool_gather_crop`` of
tests/emu_pool.py, which is sfk_u8_pool_gather_crop's -- then the emulated float stems run on it, as tests/emu_u8stem.py does for
the stacked frames.  The backend also records the names of the pool gathers it is asked for (``calls``), so a test can say
that a route launched none."""
import torch

from emu_pool import pool_gather_crop
from emu_roi_ragged import EmuRoiRaggedBackend
from video_classification_amd._lib import FMap, StemSrc
from video_classification_amd.input_pipeline import PoolClip


def materialize(x: PoolClip) -> torch.Tensor:
    """the (N, c, T, H, W) float32 clip the pooled u8 stems convolve (read at call time: follows the tables' current contents)"""
    v = pool_gather_crop(x.arena, x.index, x.lut, x.fill, x.crop, x.pad, x.c0, x.c)      # (n, t, c, h, w), the gather's memory
    return v.permute(0, 2, 1, 3, 4)


class EmuU8StemPoolBackend(EmuRoiRaggedBackend):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def u8_pool_gather(self, *a, **kw):
        self.calls.append("u8_pool_gather")
        return super().u8_pool_gather(*a, **kw)

    def u8_pool_gather_crop(self, *a, **kw):
        self.calls.append("u8_pool_gather_crop")
        return super().u8_pool_gather_crop(*a, **kw)

    @staticmethod
    def _float(p: StemSrc) -> StemSrc:
        assert isinstance(p.src, PoolClip)
        return StemSrc(materialize(p.src), p.t_index, p.kt)

    def u8pstem_conv_fwd(self, p: StemSrc, w, y: FMap, stats):
        return lambda stream: self.stem_conv_fwd(self._float(p), w, y, stats)(stream)

    def u8pstem_conv_wgrad(self, p: StemSrc, dy: FMap, dw):
        return lambda stream: self.stem_conv_wgrad(self._float(p), dy, dw)(stream)

    def u8pstem2d_fwd(self, p: StemSrc, w, y: FMap, stats):
        return lambda stream: self.stem2d_fwd(self._float(p), w, y, stats)(stream)

    def u8pstem2d_wgrad(self, p: StemSrc, dy: FMap, dw):
        return lambda stream: self.stem2d_wgrad(self._float(p), dy, dw)(stream)
