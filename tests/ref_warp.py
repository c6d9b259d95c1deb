"""References for sfk_u8_pool_gather_warp (include/sfk_warp.h) in plain torch, and the ONE set of checks that both the GPU test
(tests/test_gpu_warp.py, against the kernel) and the CPU test (tests/test_warp_cpu.py, against the emulation and its mutants)
run.

``warp32``  the header's contract in float32 torch ops.  Every torch elementwise op rounds once, so this is the bit-level
            statement of the contract: the kernel and the emulation are compared to it with torch.equal.
``warp64``  F.grid_sample(bilinear, zeros, align_corners=False) of the normalised frames in float64, the grid formed from the
            fp32 matrix cast to double as gx = (2 xs + 1) / w - 1.  It pins warp32 to the sampling everybody knows.

The bound of warp32 against warp64 (``bound``), derived, not measured.  Write u = 2^-24 and D = lut[255] - lut[0], the largest
difference between two taps (the zero of the padding lies between lut[0] and lut[255]).
 1. xs = fl(fl(fl(a x) + fl(b y)) + c) takes three roundings (x, y and the fp32 matrix are exact in both references), each at
    most half an ulp of its own result.  With Cx the largest magnitude any of a x, b y, a x + b y and xs reaches in the case,
    every result lies below the next power of two above Cx, so each rounding is at most hu(Cx) = 2^(floor(log2 Cx) - 24) and
    |xs32 - xs64| <= 3 hu(Cx); the same for ys with Cy.  (The double side's roundings, the grid's round trip included, are
    2^-29 of these.)
 2. The sampled value is a continuous function of (xs, ys) on the whole plane -- bilinear inside a cell, equal on both sides of
    a cell border, and running into the padding's zeros at xs = -1 and xs = w, where the range test cuts -- with
    |d/dxs| = |(1 - fy)(v01 - v00) + fy (v11 - v10)| <= D and likewise |d/dys| <= D.  So the coordinate errors move the value
    by at most D (3 hu(Cx) + 3 hu(Cy)).  fx = xs - floor(xs) is exact.
 3. The interpolation itself is nine fp32 operations (two differences, two products, two sums for top and bot; one of each for
    the result), every result at most D in magnitude, so at most u D each: 9 u D, counted in full although top's and bot's
    errors enter the result with weights that sum to one.
bound = 3 D (hu(Cx) + hu(Cy)) + 9 u D, with Cx, Cy taken from the case's own coordinates (all of its pixels, inflated by 2^-20
so that an fp32 result just across a power of two is covered).  For |coordinates| < 512: 3 * 4.444 * 2 * 2^-16 + 2.4e-6 =
4.1e-4.
"""
import math

import torch
import torch.nn.functional as F

from video_classification_amd.input_pipeline import draw_affine, normalize_lut

U = 2.0 ** -24
MUTANTS = ("round", "clamp", "miss0", "swap", "c0")


def _frames(pool, index):
    """(pool (F,H,W,P), index (n,t) long): a stacked (N,T,H,W,P) batch with index None is the pool of its own frames"""
    if index is None:
        n, t = pool.shape[:2]
        return pool.reshape((n * t,) + tuple(pool.shape[2:])), torch.arange(n * t).view(n, t)
    return pool, index.long()


def _values(pool, index, lut, fill, c0, c, missing_is_zero=False):
    """(n, t, h, w, c) of lut dtype: the normalised frames of the table, a missing one (index outside [0, F)) as lut[fill]"""
    f = pool.shape[0]
    miss = (index < 0) | (index >= f)
    v = lut[pool[index.clamp(0, f - 1)][..., c0:c0 + c].long()]
    fv = torch.zeros((), dtype=lut.dtype) if missing_is_zero else lut[fill]
    return torch.where(miss[:, :, None, None, None], fv, v)


def warp32(pool, index, lut, fill, warp, c0=0, c=None, mutant=None):
    """The contract of include/sfk_warp.h, op for op in float32: (n, t, c, h, w) float32.  pool (F,H,W,P) uint8 with index
    (n,t) int32, or the stacked (N,T,H,W,P) batch with index None; warp (n, 6), any values.  mutant: one of MUTANTS -- a wrong
    kernel the checks must refuse (tests/emu_warp.py)."""
    assert mutant is None or mutant in MUTANTS, mutant
    pool, index = _frames(pool, index)
    _, h, w, p = pool.shape
    c = p - c0 if c is None else c
    n = index.shape[0]
    v = _values(pool, index, lut.float(), fill, 0 if mutant == "c0" else c0, c, mutant == "miss0")
    m = warp.detach().to("cpu", torch.float32)
    if mutant == "swap":
        m = m[:, [3, 4, 5, 0, 1, 2]]
    x = torch.arange(w, dtype=torch.float32)[None, None, :]
    y = torch.arange(h, dtype=torch.float32)[None, :, None]
    k = [m[:, i][:, None, None] for i in range(6)]
    xs = (k[0] * x + k[1] * y) + k[2]                          # (n, h, w); each op one fp32 rounding
    ys = (k[3] * x + k[4] * y) + k[5]
    inr = (xs > -1) & (xs < w) & (ys > -1) & (ys < h)          # a NaN fails it
    xs, ys = torch.where(inr, xs, torch.zeros(())), torch.where(inr, ys, torch.zeros(()))
    x0f, y0f = (torch.round(xs), torch.round(ys)) if mutant == "round" else (torch.floor(xs), torch.floor(ys))
    fx, fy = (xs - x0f)[..., None, None], (ys - y0f)[..., None, None]
    x0, y0 = x0f.long(), y0f.long()                            # only after the range test
    ni = torch.arange(n)[:, None, None]

    def tap(yy, xx):                                           # (n, h, w, t, c)
        g = v[ni, :, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
        if mutant == "clamp":
            return g
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return torch.where(ok[..., None, None], g, torch.zeros(()))
    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = v00 + fx * (v01 - v00)
    bot = v10 + fx * (v11 - v10)
    out = top + fy * (bot - top)
    out = torch.where(inr[..., None, None], out, torch.zeros(()))
    return out.permute(0, 3, 4, 1, 2).contiguous()


def warp64(pool, index, lut, fill, warp, c0=0, c=None):
    """F.grid_sample(bilinear, zeros, align_corners=False) of the normalised frames in float64: (n, t, c, h, w) float64"""
    pool, index = _frames(pool, index)
    _, h, w, p = pool.shape
    c = p - c0 if c is None else c
    n, t = index.shape
    v = _values(pool, index, lut.double(), fill, c0, c).permute(0, 1, 4, 2, 3).reshape(n, t * c, h, w)
    xs, ys = coords64(warp, h, w)[:2]
    grid = torch.stack([(2 * xs + 1) / w - 1, (2 * ys + 1) / h - 1], -1)
    return F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(n, t, c, h, w)


def coords64(warp, h, w):
    """(xs, ys, Cx, Cy): the float64 source positions (n, h, w) of the fp32 matrices cast to double, and the largest magnitude
    that a x, b y, a x + b y or xs (resp. the ys terms) reaches over all pixels of all clips"""
    m = warp.detach().to("cpu", torch.float32).double()
    x = torch.arange(w, dtype=torch.float64)[None, None, :]
    y = torch.arange(h, dtype=torch.float64)[None, :, None]
    k = [m[:, i][:, None, None] for i in range(6)]
    xs, ys = k[0] * x + k[1] * y + k[2], k[3] * x + k[4] * y + k[5]
    big = lambda *ts: max(float(t.abs().max()) for t in ts)
    return xs, ys, big(k[0] * x, k[1] * y, k[0] * x + k[1] * y, xs), big(k[3] * x, k[4] * y, k[3] * x + k[4] * y, ys)


def half_ulp(cmax: float) -> float:
    """the largest rounding error of an fp32 result of magnitude at most cmax: 2^(floor(log2 cmax) - 24)"""
    cmax = max(cmax * (1 + 2.0 ** -20), 2.0 ** -100)
    return 2.0 ** (math.frexp(cmax)[1] - 1 - 24)


def bound(warp, h, w, lut) -> float:
    """the derived bound of |warp32 - warp64| for these matrices on h x w frames (module docstring)"""
    _, _, cx, cy = coords64(warp, h, w)
    d = float(lut[255] - lut[0])
    return 3 * d * (half_ulp(cx) + half_ulp(cy)) + 9 * U * d


# ---------------------------------------------------------------------------------------------------------------------------
# The checks.  A case is everything one launch needs; ``check`` compares what ``gather`` wrote to warp32, bit for bit.
# gather(pool, index | None, lut, fill, warp, c0, c, out_dtype) -> (n, t, c, h, w) tensor of out_dtype on the CPU.
TILE_H, TILE_W = 16, 32                                        # include/sfk_warp.h SFK_WARP_TILE_H / _W
FILL = 127
EXTENTS = [(TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (24, 17), (48, 40)]   # (h, w)
RANGES = [(0, 5), (5, 15), (0, 21), (20, 1)]                   # (c0, c) at pixel pitch 21
MINIFY = [3.0, 0.0, 0.0, 0.0, 3.0, 0.0]                        # reads a 3x larger box: at (48, 40) it cannot be staged
MINIFY_ROTATED = [1.75, 1.75, -20.0, -1.75, 1.75, 30.0]        # 45 degrees at 2.5x: the first tile's box is the whole (48, 40) frame
FAR = [[1.0, 0.0, 1e6, 0.0, 1.0, -1e6], [1e6, 0.0, 1e6, 0.0, 1e6, 1e6], [1e-6, 0.0, -1e6, 0.0, 1e-6, -1e6]]


def crop_rows(h, w, pad=None):
    """the integer-translation rows (1, 0, left - pad, 0, 1, top - pad) of every corner (top, left) of [0, 2 pad]^2, and
    those (top, left) pairs"""
    pad = w // 10 if pad is None else pad
    tl = [(0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad)]
    return [[1.0, 0.0, float(left - pad), 0.0, 1.0, float(top - pad)] for top, left in tl], tl


def matrix_rows(h, w, seed=0):
    """(rows (n, 6) float32, {name: clip numbers}): identity, every corner crop offset at pad = w // 10, the flip, the
    transpose, the half-pixel shift, 16 draws of draw_affine(degrees 30, scale (0.6, 1.6), shear 10, flip 0.5), the far-out
    finite rows and the two strongly minifying ones"""
    rows, where = [], {}

    def add(name, rs):
        where[name] = list(range(len(rows), len(rows) + len(rs)))
        rows.extend(rs)
    add("identity", [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    add("crop", crop_rows(h, w)[0])
    add("flip", [[-1.0, 0.0, float(w - 1), 0.0, 1.0, 0.0]])
    add("transpose", [[0.0, 1.0, 0.0, 1.0, 0.0, 0.0]])
    add("half", [[1.0, 0.0, 0.5, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0, 1.0, -0.5]])
    g = torch.Generator().manual_seed(1000 + seed)
    add("draws", draw_affine(16, max(h, w), max(h, w) // 10, 30.0, (0.6, 1.6), 10.0, 0.5, generator=g).tolist())
    add("far", FAR)
    add("minify", [MINIFY, MINIFY_ROTATED])
    return torch.tensor(rows, dtype=torch.float32), where


def random_pool(frames, h, w, pitch=21, seed=0, row_pad=0, frame_pad=0):
    """(frames, h, w, pitch) uint8 view whose row and frame strides exceed the tight ones by row_pad and frame_pad bytes; the
    padding holds bytes of its own, so a kernel that strays into it is seen"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, 256, (frames * (h * (w * pitch + row_pad) + frame_pad),), generator=g, dtype=torch.uint8)
    return buf.as_strided((frames, h, w, pitch), (h * (w * pitch + row_pad) + frame_pad, w * pitch + row_pad, pitch, 1))


def geometry_cases():
    """n = 2, t = 3 over a pool of 3 frames with padded strides: every channel range, an index table with a repeated frame,
    a -1 and an index >= frames, and index = None over the stacked batch"""
    h, w = 24, 40
    pool = random_pool(3, h, w, seed=1, row_pad=11, frame_pad=37)
    stacked = torch.randint(0, 256, (2, 3, h, w, 21), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    g = torch.Generator().manual_seed(3)
    warp = torch.cat([draw_affine(1, w, w // 10, 30.0, (0.6, 1.6), 10.0, 0.5, generator=g),
                      torch.tensor([[1.0, 0.0, -3.0, 0.0, 1.0, 2.0]])])
    index = torch.tensor([[2, 2, -1], [0, 3, 1]], dtype=torch.int32)
    cases = {}
    for c0, c in RANGES:
        cases[f"pool_c{c0}_{c}"] = dict(pool=pool, index=index, warp=warp, c0=c0, c=c)
    cases["stacked_index_none"] = dict(pool=stacked, index=None, warp=warp, c0=0, c=21)
    cases["stacked_index_none_c5_15"] = dict(pool=stacked, index=None, warp=warp, c0=5, c=15)
    return cases


def extent_cases():
    """every extent with the whole matrix set, one clip a row, t = 2, one frame of them missing"""
    cases = {}
    for k, (h, w) in enumerate(EXTENTS):
        warp, where = matrix_rows(h, w, seed=k)
        n = warp.shape[0]
        pool = random_pool(5, h, w, seed=10 + k)
        index = (torch.arange(2 * n, dtype=torch.int32) % 5).view(n, 2)
        index[where["draws"][0], 1] = -1
        index[where["crop"][1], 0] = 5
        cases[f"extent_{h}x{w}"] = dict(pool=pool, index=index, warp=warp, c0=0, c=21, where=where)
    return cases


def all_cases():
    return {**geometry_cases(), **extent_cases()}


def check(gather, case, out_dtype=torch.float32):
    """what ``gather`` writes for the case equals warp32, bit for bit; the far-out rows give zeros.  Returns what it wrote."""
    lut = normalize_lut()
    want = warp32(case["pool"], case["index"], lut, FILL, case["warp"], case["c0"], case["c"]).to(out_dtype)
    got = gather(case["pool"], case["index"], lut, FILL, case["warp"], case["c0"], case["c"], out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, tuple(got.shape))
    if not torch.equal(got, want):
        bad = (got.float() != want.float()).nonzero()
        raise AssertionError(f"{int(bad.shape[0])} elements differ from warp32, the first at (n, t, ch, y, x) = {bad[0].tolist()}: "
                             f"{float(got.float()[tuple(bad[0])])} against {float(want.float()[tuple(bad[0])])}")
    for k in case.get("where", {}).get("far", []):
        assert not got[k].any(), f"far-out row {k} did not give zeros"
    return got


def check_all(gather, out_dtype=torch.float32):
    for name, case in all_cases().items():
        try:
            check(gather, case, out_dtype)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
