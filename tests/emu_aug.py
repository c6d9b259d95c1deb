"""EmuV2Backend plus the entry points of include/sfk_aug.h as torch ops: sfk_color_jitter through tests/ref_jitter.py in
float32, written back in place in the clip's dtype."""
import torch

from emu_v2 import EmuV2Backend
from ref_jitter import ref_jitter


class EmuAugBackend(EmuV2Backend):
    def color_jitter_workspace_bytes(self, n: int, t: int, h: int, w: int) -> int:
        units = h * ((w + 7) // 8)
        return n * t * ((units + 511) // 512) * 4

    def color_jitter(self, clip, params, workspace, c_off: int = 0, bgr: bool = False, mean: float = 0.0, std: float = 1.0):
        assert clip.dim() == 5 and tuple(params.shape) == (clip.shape[0], 8) and params.dtype == torch.float32

        def run(stream):
            rgb = clip[:, :, c_off:c_off + 3]
            rgb.copy_(ref_jitter(rgb.to(torch.float32), params, 0, bgr, mean, std))
        return run
