"""EmuBackend plus the two entry points of include/sfk_stem2d.h (the frames-as-channels stem of res2d) as torch ops, so that
the res2d network runs on the engine's CPU schedule.  The contract restated: the clip is an (N, C, T, H, W) view, input
channel t*C + c of the Conv2d(T*C, cout, 7, 2, 3) = frame t, channel c; one output frame; filter in the stem layout
[co][((t*C + c)*7 + kh)*8 + kw]; BatchNorm partial sums per 16x16 tile; the filter gradient overwrites dw."""
import torch

from emu_backend import EmuBackend
from video_classification_amd._lib import FMap, StemSrc, stem_kp


def stem2d_ref(x5: torch.Tensor, w: torch.Tensor, cout: int) -> torch.Tensor:
    """x5 (N, C, T, H, W) fp32, w the stem layout -> (N, cout, 1, Ho, Wo)"""
    t, c = x5.shape[2], x5.shape[1]
    wt = EmuBackend.stem_weight_from_layout(w.float(), cout, c, t)
    return torch.nn.functional.conv3d(x5, wt, None, (1, 2, 2), (0, 3, 3))


class EmuStem2dBackend(EmuBackend):
    def stem2d_tiles(self, p: StemSrc, y: FMap) -> int:
        assert y.t == 1
        return y.n * ((y.h + 15) // 16) * ((y.w + 15) // 16)

    def stem2d_fwd(self, p: StemSrc, w, y: FMap, stats):
        def run(stream):
            x = p.src.to(y.dtype).float()           # the clip is rounded to the compute precision when staged
            out = stem2d_ref(x, w, y.c)
            y.view5().copy_(out.permute(0, 2, 3, 4, 1).to(y.dtype))
            if stats is not None:
                mt = self.stem2d_tiles(p, y)
                st = stats[: mt * y.c * 2].view(mt, y.c, 2)
                st.zero_()
                st[0, :, 0] = out.sum((0, 2, 3, 4))
                st[0, :, 1] = (out * out).sum((0, 2, 3, 4))
        return run

    def stem2d_wgrad(self, p: StemSrc, dy: FMap, dw):
        def run(stream):
            x = p.src.to(dy.dtype).float()
            cin, t, cout = x.shape[1], x.shape[2], dy.c
            with torch.enable_grad():
                wt = torch.zeros(cout, cin, t, 7, 7, requires_grad=True)
                out = torch.nn.functional.conv3d(x.detach(), wt, None, (1, 2, 2), (0, 3, 3))
                out.backward(dy.view5().float().permute(0, 4, 1, 2, 3))
            kp = stem_kp(cin, t)
            g = torch.nn.functional.pad(wt.grad.permute(0, 2, 1, 3, 4), (0, 1)).reshape(cout, t * cin * 7 * 8)
            d = dw[: cout * kp].view(cout, kp)
            d.zero_()
            d[:, : g.shape[1]] = g
        return run
