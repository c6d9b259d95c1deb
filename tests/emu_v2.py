"""EmuU8StemBackend plus the two entry points of include/sfk_v2.h as torch ops: sfk_roi_resize through
F.interpolate on the clamped box (then the RandomCrop shift), sfk_sgd through torch.optim.SGD's single-tensor update."""
import torch
import torch.nn.functional as F

from emu_u8stem import EmuU8StemBackend


def clamp_box(b, h: int, w: int):
    """the box the kernel reads: clamped the way a Python slice clamps it (include/sfk_v2.h)"""
    x1, y1, x2, y2 = (int(v) for v in b)
    x1, y1 = min(max(x1, 0), w - 1), min(max(y1, 0), h - 1)
    return x1, y1, min(max(x2, x1 + 1), w), min(max(y2, y1 + 1), h)


def roi_resize_ref(src, lut, box, out_h: int, out_w: int, antialias: bool, crop=None, pad: int = 0) -> torch.Tensor:
    """src (N,T,H,W,C) uint8 -> (N,T,C,out_h,out_w) float32, the header's formula"""
    n, t, h, w, c = src.shape
    res = torch.empty(n, t, c, out_h, out_w)
    for i in range(n):
        x1, y1, x2, y2 = clamp_box(box[i].tolist(), h, w)
        v = lut.cpu()[src[i, :, y1:y2, x1:x2, :].long().cpu()].permute(0, 3, 1, 2)       # t c h w
        r = F.interpolate(v.reshape(t * c, 1, y2 - y1, x2 - x1), (out_h, out_w), mode="bilinear", align_corners=False,
                          antialias=antialias).reshape(t, c, out_h, out_w)
        if crop is not None:
            top, left = int(crop[i, 0]) - pad, int(crop[i, 1]) - pad
            sh = torch.zeros_like(r)
            ys, xs = slice(max(0, -top), min(out_h, out_h - top)), slice(max(0, -left), min(out_w, out_w - left))
            yr, xr = slice(ys.start + top, ys.stop + top), slice(xs.start + left, xs.stop + left)
            if ys.start < ys.stop and xs.start < xs.stop:
                sh[:, :, ys, xs] = r[:, :, yr, xr]
            r = sh
        res[i] = r
    return res


class EmuV2Backend(EmuU8StemBackend):
    def roi_resize(self, src, lut, box, out, antialias: bool, crop=None, pad: int = 0, c_off: int = 0):
        def run(stream):
            n, t, h, w, c = src.shape
            r = roi_resize_ref(src, lut, box, out.shape[3], out.shape[4], antialias, crop, pad)
            out[:, :, c_off:c_off + c].copy_(r)
        return run

    def sgd(self, p, g, buf, count, lr, momentum, dampening, nesterov, gscale, step, shadow=None):
        def run(stream):
            step.add_(1)
            gg = g[:count] * gscale
            d = gg
            if momentum != 0:
                b = buf[:count]
                if int(step[0]) == 1:
                    b.copy_(gg)
                else:
                    b.mul_(momentum).add_(gg, alpha=1 - dampening)
                d = gg.add(b, alpha=momentum) if nesterov else b
            p[:count].add_(d, alpha=-lr)
            if shadow is not None:
                shadow[:count].copy_(p[:count])
        return run
