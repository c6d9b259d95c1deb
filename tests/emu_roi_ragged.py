"""EmuRoiPoolBackend plus the entry point of include/sfk_roi_ragged.h as torch ops: sfk_roi_resize_ragged is ``roi_resize_ref``
(tests/emu_v2.py) clip by clip on the frames MATERIALISED from the arena -- the header's own statement of the contract."""
import torch

from emu_roi_pool import EmuRoiPoolBackend
from emu_v2 import roi_resize_ref


def materialise_ragged(arena, offset, hw, fill: int, max_hw, pitch: int = 7, c0: int = 0, c=None):
    """one clip: (1, T, h, w, c) uint8, frame t the h x w pixels of ``pitch`` packed bytes at arena[offset[t]:], channels
    c0 .. c0+c-1; bytes of fill for a frame that does not lie in the arena whole or whose (h, w) is outside [1, max_hw] -- the
    rectangle is then (h, w) clamped into that range, as the header says"""
    c = pitch - c0 if c is None else c
    hn, wn = (int(v) for v in hw)
    h, w = min(max(hn, 1), int(max_hw[0])), min(max(wn, 1), int(max_hw[1]))
    a = arena.cpu()
    frames = []
    for o in (int(v) for v in offset):
        if o >= 0 and (hn, wn) == (h, w) and o + h * w * pitch <= a.numel():
            frames.append(a[o:o + h * w * pitch].view(h, w, pitch)[..., c0:c0 + c])
        else:
            frames.append(torch.full((h, w, c), fill, dtype=torch.uint8))
    return torch.stack(frames)[None]


class EmuRoiRaggedBackend(EmuRoiPoolBackend):
    def roi_resize_ragged(self, arena, offset, hw, lut, fill, box, out, antialias, crop=None, pad=0, pitch=7, c0=0, c=None,
                          c_off=0, max_hw=None):
        c = pitch - c0 if c is None else c
        n, t = offset.shape
        assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.numel() % 4 == 0 and arena.data_ptr() % 4 == 0
        assert offset.dtype == torch.int64 and hw.dtype == torch.int32 and box.dtype == torch.int32
        assert tuple(hw.shape) == (n, 2) and tuple(box.shape) == (n, 4) and tuple(out.shape[:2]) == (n, t) and c_off + c <= out.shape[2]
        assert crop is None or (crop.dtype == torch.int32 and tuple(crop.shape) == (n, 2))
        if max_hw is None:
            max_hw = tuple(max(int(v), 1) for v in hw.max(0).values.tolist())

        def run(stream):
            for i in range(n):
                clip = materialise_ragged(arena, offset[i], hw[i], fill, max_hw, pitch, c0, c)
                r = roi_resize_ref(clip, lut, box[i:i + 1], out.shape[3], out.shape[4], antialias,
                                   None if crop is None else crop[i:i + 1], pad)
                out[i:i + 1, :, c_off:c_off + c].copy_(r)
        return run
