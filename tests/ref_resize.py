"""The arithmetic of sfk_u8_pad_resize_cubic (include/sfk_resize.h), written out independently in numpy: the integer
definition (ints as int64, floats as np.float32, every float operation rounded on its own -- numpy does not contract) and the
real cubic in float64 it approximates.  cv2 is not installed here: this file, not cv2.resize, is what the kernel is pinned to."""
import numpy as np

F32 = np.float32
A = F32(-0.75)


def pad_geometry(h, w):
    m = max(h, w)
    return m, (m - w) // 2, (m - h) // 2


def pad_square(img):
    """(h, w, c) -> the (m, m, c) zero-padded square about its centre"""
    h, w, c = img.shape
    m, nx, ny = pad_geometry(h, w)
    sq = np.zeros((m, m, c), dtype=img.dtype)
    sq[ny:ny + h, nx:nx + w] = img
    return sq


def axis_table(m, size):
    """per output coordinate d: the clipped tap positions (size, 4) int64, the 11-bit coefficients (size, 4) int64 and the
    unclipped s (size,) int64"""
    d = np.arange(size, dtype=np.float64)
    f = ((d + 0.5) * (float(m) / size) - 0.5).astype(F32)                     # the expression in double, then float32
    fl = np.floor(f)
    t = (f - fl).astype(F32)
    s = fl.astype(np.int64)
    one, two, three, four, five, eight = (F32(v) for v in (1, 2, 3, 4, 5, 8))
    u = t + one
    k0 = ((A * u - five * A) * u + eight * A) * u - four * A
    k1 = ((A + two) * t - (A + three)) * t * t + one
    v = one - t
    k2 = ((A + two) * v - (A + three)) * v * v + one
    k3 = one - k0 - k1 - k2
    k = np.stack([k0, k1, k2, k3], axis=1)
    assert k.dtype == F32 and u.dtype == F32
    q = np.rint(k * F32(2048)).astype(np.int64)                               # round half to even
    taps = np.clip(s[:, None] - 1 + np.arange(4)[None, :], 0, m - 1)
    return taps, q, s


def pad_resize_int(img, size, unclamped=False):
    """(h, w, c) uint8 -> (size, size, c) uint8 by the integer definition; unclamped=True: (V + 2^21) >> 22 before the clamp"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    sq = pad_square(img).astype(np.int64)
    m = sq.shape[0]
    taps, q, _ = axis_table(m, size)
    rows = np.einsum("yi,yimc->ymc", q, sq[taps])                             # (size, m, c): rows first
    v = np.einsum("xj,yxjc->yxc", q, rows[:, taps])                           # (size, size, c)
    assert int(np.abs(v).max(initial=0)) < 2 ** 31
    r = (v + (1 << 21)) >> 22                                                 # arithmetic shift
    return r if unclamped else np.clip(r, 0, 255).astype(np.uint8)


def pad_resize_f64(img, size):
    """the real cubic in float64: same A, same taps, exact coefficients, round half to even, clamp"""
    img = np.asarray(img)
    sq = pad_square(img).astype(np.float64)
    m = sq.shape[0]
    d = np.arange(size, dtype=np.float64)
    f = (d + 0.5) * (float(m) / size) - 0.5
    s = np.floor(f)
    t = f - s
    a = -0.75
    k = np.stack([((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a, ((a + 2) * t - (a + 3)) * t * t + 1,
                  ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1], axis=1)
    k = np.concatenate([k, 1 - k.sum(axis=1, keepdims=True)], axis=1)
    taps = np.clip(s.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, m - 1)
    rows = np.einsum("yi,yimc->ymc", k, sq[taps])
    v = np.einsum("xj,yxjc->yxc", k, rows[:, taps])
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def floors_agree(h, w, size):
    """the float32 floor of the coordinate equals the float64 floor for every output coordinate of this shape"""
    m = max(h, w)
    f = (np.arange(size, dtype=np.float64) + 0.5) * (float(m) / size) - 0.5
    return bool(np.array_equal(np.floor(f.astype(F32)).astype(np.int64), np.floor(f).astype(np.int64)))


def resize_table(src, offset, hw, c, size, max_side, fill):
    """the whole launch: src 1-D uint8, offset (F,), hw (F, 2) -> (F, size, size, c) uint8, a missing frame as bytes of fill"""
    src = np.asarray(src)
    out = np.empty((len(offset), size, size, c), dtype=np.uint8)
    for i, (off, (h, w)) in enumerate(zip(np.asarray(offset).tolist(), np.asarray(hw).tolist())):
        if h <= 0 or w <= 0 or h > max_side or w > max_side or off < 0 or off + h * w * c > src.shape[0]:
            out[i] = fill
        else:
            out[i] = pad_resize_int(src[off:off + h * w * c].reshape(h, w, c), size)
    return out
