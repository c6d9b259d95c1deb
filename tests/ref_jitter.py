"""torchvision's float-tensor ColorJitter.forward, restated once in plain torch (torchvision is not installed here: the
semantics are its documented ones -- functional adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue with
_blend, rgb_to_grayscale, _rgb2hsv and _hsv2rgb -- "parity unpinned" against torchvision itself).  Every function works in
the float dtype it is given; the tests use float32 (what the kernel computes in) and float64 (the reference)."""
import torch


def gray(img):
    r, g, b = img.unbind(-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def blend(a, b, f):
    return (f * a + (1 - f) * b).clamp(0, 1)


def rgb2hsv(img):
    r, g, b = img.unbind(-3)
    maxc, minc = img.max(-3).values, img.min(-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    crd = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc), -3)


def hsv2rgb(img):
    h, s, v = img.unbind(-3)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    sel = lambda six: sum((i == k).to(img.dtype) * six[k] for k in range(6))
    return torch.stack((sel((v, q, p, p, t, v)), sel((t, v, v, q, p, p)), sel((p, p, t, v, v, q))), -3)


def adjust_hue(img, hf):
    hsv = rgb2hsv(img)
    h, s, v = hsv.unbind(-3)
    return hsv2rgb(torch.stack(((h + hf) % 1.0, s, v), -3))


def jitter_rgb(img, params):
    """img (..., T, 3, H, W) in image units, planes R, G, B; params (8,) = order[4], b, c, s, h: ColorJitter.forward with
    those draws, one set for every frame.  An order entry outside 0..3 skips its slot."""
    p = params.to(img.dtype)
    for slot in range(4):
        op = int(params[slot])
        if op == 0:
            img = blend(img, torch.zeros_like(img), p[4])
        elif op == 1:
            img = blend(img, gray(img).mean(dim=(-3, -2, -1), keepdim=True), p[5])      # per frame
        elif op == 2:
            img = blend(img, gray(img), p[6])
        elif op == 3:
            img = adjust_hue(img, p[7])
    return img


def ref_jitter(clip, params, c_off: int = 0, bgr: bool = False, mean: float = 0.0, std: float = 1.0):
    """include/sfk_aug.h on a copy: clip (N, T, C, H, W) of any float dtype, channels c_off .. c_off+2 jittered per clip with
    params (N, 8), every other channel untouched.  mean and std are taken as the float32 values the descriptor carries."""
    out = clip.clone()
    dt = clip.dtype
    m = torch.tensor(mean, dtype=torch.float32).to(dt)
    s = torch.tensor(std, dtype=torch.float32).to(dt)
    for i in range(clip.shape[0]):
        v = clip[i, :, c_off:c_off + 3] * s + m
        if bgr:
            v = v.flip(-3)
        v = jitter_rgb(v, params[i].to(torch.float32).cpu())
        if bgr:
            v = v.flip(-3)
        out[i, :, c_off:c_off + 3] = (v - m) / s
    return out
