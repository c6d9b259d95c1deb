"""References for sfk_roi_resize_warp / _pool_warp / _ragged_warp (include/sfk_roi_warp.h) in plain torch, and the ONE set of
cases and checks that both the GPU test (tests/test_gpu_roi_warp.py, against the kernel) and the CPU test
(tests/test_roi_warp_cpu.py, against the emulation and its mutants) run.

``roi_warp32``  the header's contract in float32 and float64 torch ops, op for op.  Every torch elementwise op rounds once, so
                this is the bit-level statement of the contract: the kernel and the emulation are compared to it with
                torch.equal.  (The fused operations, fma(scale, u + 0.5, -0.5) and every tap after the first of a weighted
                sum, are formed in float64 -- the 24 x 24 bit product is exact there -- and rounded once to float32.)
``roi_warp64``  the same positions -- u and v are the contract's fp32-rounded ones, so both references zero the same pixels --
                with the interpolant in float64: exact scale in / out, exact triangle weights, float64 sums.

The bound of roi_warp32 against roi_warp64 (``bound``), derived from the count of rounded operations, not measured.  Write
u = 2^-24, hu(c) = 2^(floor(log2 c) - 24) (the largest rounding error of an fp32 result of magnitude at most c) and V =
max |lut|.  Per axis, with `in` the box extent and K the number of taps (2 without antialiasing, 2 ceil(support) + 1 with):
 1. the tap position (src, or center) is fl(scale) times an exact factor, rounded once: fl(scale) is off by at most 2^-24
    relative, which moves the position by at most in * 2^-24 <= 2 hu(in), and the rounding adds hu(in): delta = 3 hu(in).
    Every weight is a function of the position with slope at most 1 (the triangle's slope is invscale <= 1), so delta moves a
    weight by at most delta.  (A tap that enters or leaves the window because of it has weight at most delta there.)
 2. antialias = 0: src - i0 is exact (both lie within 1 of each other), l0 = 1 - l1 rounds once: each weight is off by at
    most delta + 2 u, E = 2 (delta + 2 u) summed over the two taps.
    antialias = 1: (k + xmin) - center rounds once at magnitude <= K (hu(K)); the product with invscale, invscale itself and
    1 - x round once each at magnitude <= 1 (3 u); so a raw weight is off by at most e = delta + hu(K) + 3 u.  The total of up
    to K raw weights takes K - 1 additions at magnitude <= K ((K - 1) hu(K)) and is at least 1/2 (the window holds the
    centre's own pixel or both its neighbours), the quotient rounds once more: a normalised weight w / total is off by at most
    2 e + 2 w (K e + (K - 1) hu(K)) + u, and over the K weights (which sum to 1): E = 2 K e + 2 (K e + (K - 1) hu(K)) + K u
    <= 4 K (e + hu(K)) + K u.
 3. the result is sum_r wy_r sum_k wx_k lut[..]: the weight errors move it by at most V (E_x + E_y) (the other axis' weights
    sum to at most 1 + E), and the roundings of the products and sums (K_x + K_y with the fused taps; counted as if every
    product and sum rounded on its own, 2 K_x - 1 + 2 K_y - 1), each of a value at most V, add at most 2 (K_x + K_y) u V.
bound = V (E_x + E_y) + 2 (K_x + K_y) u V, the worst box of the case.  For a 39 x 54 box to 13 x 18 with antialiasing (K = 7):
about 3.6e-4; without, about 2.4e-5.
"""
import math

import torch

from video_classification_amd.input_pipeline import byte_lut, draw_affine, stream_of

U = 2.0 ** -24
MUTANTS = ("round", "blend", "miss0", "swap", "support", "c_off")
TILE_H, TILE_W = 16, 32                                        # include/sfk_roi_warp.h SFK_ROI_WARP_TILE_H / _W
STAGE_BYTES = 24 * 1024                                        # include/sfk_roi_warp.h SFK_ROI_WARP_LDS_BYTES
FILL = 93


def clamp_box(b, h: int, w: int):
    """the box the kernel reads: clamped the way a Python slice clamps it (include/sfk_v2.h)"""
    x1, y1, x2, y2 = (int(v) for v in b)
    x1, y1 = min(max(x1, 0), w - 1), min(max(y1, 0), h - 1)
    return x1, y1, min(max(x2, x1 + 1), w), min(max(y2, y1 + 1), h)


def positions(warp, out_h: int, out_w: int, swap: bool = False):
    """(u, v, ok): the contract's fp32 positions (n, out_h, out_w) and its range test"""
    m = warp.detach().to("cpu", torch.float32)
    if swap:
        m = m[:, [3, 4, 5, 0, 1, 2]]
    x = torch.arange(out_w, dtype=torch.float32)[None, None, :]
    y = torch.arange(out_h, dtype=torch.float32)[None, :, None]
    k = [m[:, i][:, None, None] for i in range(6)]
    u = (k[0] * x + k[1] * y) + k[2]                           # each op one fp32 rounding
    v = (k[3] * x + k[4] * y) + k[5]
    ok = (u >= -0.5) & (u <= out_w - 0.5) & (v >= -0.5) & (v <= out_h - 0.5)      # a NaN fails it
    return u, v, ok


def _taps32(p, inn: int, out: int, aa: bool, mutant=None, widen: float = 1.0):
    """the header's taps of fp32 positions p (any shape, all inside the range test) -> (idx (..., K) long, wt (..., K) f32);
    taps past a pixel's own count have weight 0 (they cannot change a value)"""
    f32, f64 = torch.float32, torch.float64
    scale = torch.tensor(float(inn), dtype=f32) / torch.tensor(float(out), dtype=f32)
    if not aa:
        src = (scale.to(f64) * (p + 0.5).to(f64) - 0.5).to(f32)                  # fma: one rounding
        src = torch.where(src < 0, torch.zeros((), dtype=f32), src)
        i0 = (torch.round(src) if mutant == "round" else torch.floor(src)).clamp(max=inn - 1)
        l1 = (src - i0).clamp(0, 1)
        i0 = i0.long()
        i1 = i0 + (i0 < inn - 1).long()
        return torch.stack([i0, i1], -1), torch.stack([1 - l1, l1], -1)
    support = scale if float(scale) >= 1 else torch.ones((), dtype=f32)
    invscale = (1.0 / scale.to(f64)).to(f32) if float(scale) >= 1 else torch.ones((), dtype=f32)
    if mutant == "support":                                    # the matrix's own minification widens the filter
        support = support * torch.tensor(max(1.0, widen), dtype=f32)
        invscale = (1.0 / support.to(f64)).to(f32)
    center = (scale.to(f64) * (p.to(f64) + 0.5)).to(f32)
    xmin = ((center - support).to(f64) + 0.5).trunc().long().clamp(min=0)
    xmax = ((center + support).to(f64) + 0.5).trunc().long().clamp(max=inn)
    xsize = (xmax - xmin).clamp(0, int(math.ceil(float(support))) * 2 + 1)
    kk = torch.arange(max(int(xsize.max()), 1))
    x = ((((kk + xmin[..., None]).to(f32) - center[..., None]).to(f64) + 0.5) * invscale.to(f64)).to(f32).abs()
    w = torch.where(x < 1, (1.0 - x.to(f64)).to(f32), torch.zeros((), dtype=f32))
    w = torch.where(kk < xsize[..., None], w, torch.zeros((), dtype=f32))
    total = torch.zeros_like(center)
    for k in range(kk.numel()):
        total = total + w[..., k]
    w = torch.where((total != 0)[..., None], w / total[..., None], w)
    return (xmin[..., None] + kk).clamp(0, inn - 1), w


def _taps64(p, inn: int, out: int, aa: bool):
    """the same interpolant in exact arithmetic carried out in float64"""
    f64 = torch.float64
    p = p.to(f64)
    scale = inn / out
    if not aa:
        src = (scale * (p + 0.5) - 0.5).clamp(min=0)
        i0 = torch.floor(src).clamp(max=inn - 1)
        l1 = (src - i0).clamp(0, 1)
        i0 = i0.long()
        return torch.stack([i0, i0 + (i0 < inn - 1).long()], -1), torch.stack([1 - l1, l1], -1)
    support = max(scale, 1.0)
    center = scale * (p + 0.5)
    xmin = (center - support + 0.5).trunc().long().clamp(min=0)
    xmax = (center + support + 0.5).trunc().long().clamp(max=inn)
    xsize = (xmax - xmin).clamp(0, int(math.ceil(support)) * 2 + 1)
    kk = torch.arange(max(int(xsize.max()), 1))
    x = ((kk + xmin[..., None]).to(f64) - center[..., None] + 0.5).abs() / support
    w = (1 - x).clamp(min=0) * (kk < xsize[..., None])
    tot = w.sum(-1, keepdim=True)
    return (xmin[..., None] + kk).clamp(0, inn - 1), torch.where(tot != 0, w / tot, w)


def _mac(a, b, acc):
    """the contract's weighted sum, one tap: a * b for the first, fma(a, b, acc) after it.  The fp32 fma is formed in float64,
    where the 24 x 24 bit product is exact, and rounded to float32; float64 operands (roi_warp64) are plain arithmetic"""
    if acc is None:
        return a * b
    if a.dtype == torch.float64:
        return acc + a * b
    return (a.double() * b.double() + acc.double()).float()


def _sample(src, lut, box, warp, out_h, out_w, antialias, missing, fill, mutant, exact):
    n, t, h, w, c = src.shape
    dt = torch.float64 if exact else torch.float32
    lut = lut.detach().cpu().to(dt)
    u, v, ok = positions(warp, out_h, out_w, swap=mutant == "swap")
    if mutant == "blend":                                      # a soft edge: valid a half pixel further out, ramped to zero
        ok = (u > -1) & (u < out_w) & (v > -1) & (v < out_h)
    zero = torch.zeros((), dtype=torch.float32)
    res = torch.zeros(n, t, c, out_h, out_w, dtype=dt)
    m = warp.detach().to("cpu", torch.float32)
    for i in range(n):
        x1, y1, x2, y2 = clamp_box(box[i].tolist(), h, w)
        bh, bw = y2 - y1, x2 - x1
        val = lut[src[i, :, y1:y2, x1:x2, :].long().cpu()]                       # t bh bw c
        if missing is not None:
            fv = torch.zeros((), dtype=dt) if mutant == "miss0" else lut[fill]
            val = torch.where(missing[i][:, None, None, None], fv, val)
        ui, vi = torch.where(ok[i], u[i], zero), torch.where(ok[i], v[i], zero)
        if mutant == "blend":
            ui, vi = ui.clamp(-0.5, out_w - 0.5), vi.clamp(-0.5, out_h - 0.5)
        if exact:
            xi, xw = _taps64(ui, bw, out_w, antialias)
            yi, yw = _taps64(vi, bh, out_h, antialias)
        else:
            xi, xw = _taps32(ui, bw, out_w, antialias, mutant, float(m[i, [0, 1]].abs().sum()))
            yi, yw = _taps32(vi, bh, out_h, antialias, mutant, float(m[i, [3, 4]].abs().sum()))
        acc = None
        for r in range(yi.shape[-1]):
            hrow = None
            for k in range(xi.shape[-1]):
                hrow = _mac(val[:, yi[..., r], xi[..., k], :], xw[..., k][None, :, :, None], hrow)          # t oh ow c
            acc = _mac(hrow, yw[..., r][None, :, :, None], acc)
        if mutant == "blend":
            ramp = (u[i] + 1).clamp(0, 1) * (out_w - u[i]).clamp(0, 1) * (v[i] + 1).clamp(0, 1) * (out_h - v[i]).clamp(0, 1)
            acc = acc * ramp.nan_to_num(0.0)[None, :, :, None]
        acc = torch.where(ok[i][None, :, :, None], acc, torch.zeros((), dtype=dt))
        res[i] = acc.permute(0, 3, 1, 2)
    return res


def roi_warp32(src, lut, box, warp, out_h: int, out_w: int, antialias: bool, missing=None, fill: int = FILL, mutant=None):
    """The contract of include/sfk_roi_warp.h, op for op: src (N,T,H,W,C) uint8 (a missing frame's bytes are ignored where
    missing (N,T) bool says so: it is the constant image of byte fill), box (N,4), warp (N,6) any values -> (N,T,C,out_h,out_w)
    float32.  mutant: one of MUTANTS -- a wrong kernel the checks must refuse (tests/emu_roi_warp.py; 'c_off' is the
    backend's)."""
    assert mutant is None or mutant in MUTANTS, mutant
    return _sample(src, lut, box, warp, out_h, out_w, bool(antialias), missing, fill, mutant, False)


def roi_warp64(src, lut, box, warp, out_h: int, out_w: int, antialias: bool, missing=None, fill: int = FILL):
    """the same positions (fp32-rounded u and v) with the float64 interpolant: (N,T,C,out_h,out_w) float64"""
    return _sample(src, lut, box, warp, out_h, out_w, bool(antialias), missing, fill, None, True)


def half_ulp(cmax: float) -> float:
    """the largest rounding error of an fp32 result of magnitude at most cmax: 2^(floor(log2 cmax) - 24)"""
    cmax = max(cmax * (1 + 2.0 ** -20), 2.0 ** -100)
    return 2.0 ** (math.frexp(cmax)[1] - 1 - 24)


def _axis_error(inn: int, out: int, aa: bool):
    """(E, K) of the module docstring for one axis"""
    delta = 3 * half_ulp(inn)
    if not aa:
        return 2 * (delta + 2 * U), 2
    k = int(math.ceil(max(inn / out, 1.0))) * 2 + 1
    e = delta + half_ulp(k) + 3 * U
    return 4 * k * (e + half_ulp(k)) + k * U, k


def bound(box, h: int, w: int, out_h: int, out_w: int, antialias: bool, lut) -> float:
    """the derived bound of |roi_warp32 - roi_warp64| (module docstring), the worst of the case's boxes"""
    vmax = float(lut.abs().max())
    worst = 0.0
    for b in box.tolist():
        x1, y1, x2, y2 = clamp_box(b, h, w)
        (ex, kx), (ey, ky) = _axis_error(x2 - x1, out_w, antialias), _axis_error(y2 - y1, out_h, antialias)
        worst = max(worst, vmax * (ex + ey) + 2 * (kx + ky) * U * vmax)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# The cases.  A case is everything one launch of the stacked entry point needs.
H, W, C = 40, 56, 7
SIZES = [(TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (33, 17)]     # (out_h, out_w); the last 3 x 1 tiles
BOX_SIZE = (13, 18)                                            # the output of the box sweep: a 39 x 54 box is 3x
BOXES = {"down3": (1, 0, 55, 39), "up": (20, 15, 29, 21), "same": (7, 9, 25, 22), "thin": (30, 5, 31, 35),
         "corner": (46, 32, 56, 40), "beyond": (30, 20, 80, 60)}
FAR = [[1.0, 0.0, 1e6, 0.0, 1.0, -1e6], [1e6, 0.0, 1e6, 0.0, 1e6, 1e6], [1e-6, 0.0, -1e6, 0.0, 1e-6, -1e6]]


def random_clip(n, t, h=H, w=W, c=C, seed=0, row_pad=5, frame_pad=13):
    """(n, t, h, w, c) uint8 view with padded row and frame strides; the padding holds bytes of its own"""
    g = torch.Generator().manual_seed(seed)
    fs = h * (w * c + row_pad) + frame_pad
    buf = torch.randint(0, 256, (n * t * fs,), generator=g, dtype=torch.uint8)
    return buf.as_strided((n, t, h, w, c), (t * fs, fs, w * c + row_pad, c, 1))


def crop_rows(out_h, out_w, pad=None):
    """the integer-translation rows (1, 0, left - pad, 0, 1, top - pad) of the corners and one inner point of [0, 2 pad]^2,
    and those (top, left) pairs"""
    pad = max(out_w // 10, 1) if pad is None else pad
    tl = [(0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad), (pad, pad), (pad - 1, pad + 1)]
    return [[1.0, 0.0, float(left - pad), 0.0, 1.0, float(top - pad)] for top, left in tl], tl, pad


def matrix_rows(out_h, out_w, seed=0, draws=6):
    """(rows (n, 6) float32, {name: clip numbers}): identity, the crop rows, the flip, the transpose, half-pixel shifts,
    draws of draw_affine(degrees 30, scale (0.6, 1.6), shear 10, flip 0.5), a strongly minifying row, the far-out finite rows"""
    rows, where = [], {}

    def add(name, rs):
        where[name] = list(range(len(rows), len(rows) + len(rs)))
        rows.extend(rs)
    add("identity", [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    add("crop", crop_rows(out_h, out_w)[0])
    add("flip", [[-1.0, 0.0, float(out_w - 1), 0.0, 1.0, 0.0]])
    add("transpose", [[0.0, 1.0, 0.0, 1.0, 0.0, 0.0]])
    add("half", [[1.0, 0.0, 0.5, 0.0, 1.0, 0.0], [1.0, 0.0, -0.5, 0.0, 1.0, -0.5], [1.0, 0.0, 0.0, 0.0, 1.0, 0.5]])
    s = max(out_h, out_w)
    g = torch.Generator().manual_seed(2000 + seed)
    add("draws", draw_affine(draws, s, s // 10, 30.0, (0.6, 1.6), 10.0, 0.5, generator=g).tolist())
    add("minify", [[2.5, 0.3, -4.0, -0.3, 2.5, -2.0]])
    add("far", FAR)
    return torch.tensor(rows, dtype=torch.float32), where


def _case(out_h, out_w, box, antialias, seed, t=2):
    warp, where = matrix_rows(out_h, out_w, seed)
    n = warp.shape[0]
    return dict(src=random_clip(n, t, seed=seed), box=torch.tensor([box] * n, dtype=torch.int32), warp=warp, out_h=out_h,
                out_w=out_w, antialias=antialias, where=where)


def size_cases():
    """every output size around the tile, a downscaling and an upscaling box alternating, both antialias modes"""
    cases = {}
    for k, (oh, ow) in enumerate(SIZES):
        for aa in (False, True):
            cases[f"size_{oh}x{ow}_aa{int(aa)}"] = _case(oh, ow, BOXES["down3"] if (k + aa) % 2 == 0 else BOXES["up"], aa, 10 + k)
    return cases


def box_cases():
    cases = {}
    for k, (name, box) in enumerate(BOXES.items()):
        for aa in (False, True):
            cases[f"box_{name}_aa{int(aa)}"] = _case(BOX_SIZE[0], BOX_SIZE[1], box, aa, 30 + k)
    return cases


def global_cases():
    """a 64 x 96 x 7 box to one 16 x 32 tile: under the identity, the minifying row and a draw the tile's window is the whole
    box, 43 008 bytes > SFK_ROI_WARP_LDS_BYTES, so the workgroups take their taps from global memory"""
    h, w = 64, 96
    assert h * w * C > STAGE_BYTES
    g = torch.Generator().manual_seed(77)
    warp = torch.cat([torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [2.5, 0.3, -4.0, -0.3, 2.5, -2.0], [0.9, 0.0, 1.5, 0.0, 0.9, 0.25]]),
                      draw_affine(1, 32, 3, 30.0, (0.6, 1.6), 10.0, 0.5, generator=g)])
    n = warp.shape[0]
    return {f"global_aa{int(aa)}": dict(src=random_clip(n, 1, h, w, seed=50), box=torch.tensor([[0, 0, w, h]] * n, dtype=torch.int32),
                                        warp=warp, out_h=TILE_H, out_w=TILE_W, antialias=aa, where={}) for aa in (False, True)}


def all_cases():
    return {**size_cases(), **box_cases(), **global_cases()}


def expected32(case, mutant=None):
    return roi_warp32(case["src"], byte_lut(), case["box"], case["warp"], case["out_h"], case["out_w"], case["antialias"],
                      case.get("missing"), FILL, mutant)


# ---------------------------------------------------------------------------------------------------------------------------
# The launches.  ``backend`` is HipBackend on a GPU or the emulation on the CPU: the same methods either way.
SENTINEL = 7.5


def framed_out(n, t, c, out_h, out_w, dtype, device, planes_before=1, planes_after=1):
    """(buf, out, c_off): out is the (n, t, c + before + after, out_h, out_w) view of a larger buffer of SENTINEL -- a row
    above and below, two columns left, three right -- whose planes c_off .. c_off + c - 1 the launch writes"""
    buf = torch.full((n, t, c + planes_before + planes_after, out_h + 2, out_w + 5), SENTINEL, dtype=dtype, device=device)
    return buf, buf[:, :, :, 1:1 + out_h, 2:2 + out_w], planes_before


def read_framed(buf, out, c_off, c):
    """what the launch wrote, on the CPU; asserts that nothing else of the buffer changed"""
    got = out[:, :, c_off:c_off + c].detach().cpu().clone()
    rest = buf.detach().cpu().clone()
    rest[:, :, c_off:c_off + c, 1:1 + out.shape[3], 2:2 + out.shape[4]] = SENTINEL
    assert bool((rest == SENTINEL).all()), "the launch wrote outside its planes, rows or columns"
    return got


def sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def launch_stacked(backend, device, case, dtype=torch.float32):
    """the case through roi_resize_warp on its padded-stride source, into a framed destination"""
    src = case["src"]
    n, t, h, w, c = src.shape
    dev_src = torch.empty_strided(src.shape, src.stride(), dtype=torch.uint8, device=device)
    dev_src.copy_(src)
    buf, out, c_off = framed_out(n, t, c, case["out_h"], case["out_w"], dtype, device)
    backend.roi_resize_warp(dev_src, byte_lut().to(device), case["box"].to(device), case["warp"].to(device), out,
                            case["antialias"], c_off=c_off)(stream_of(torch.device(device)))
    sync(device)
    return read_framed(buf, out, c_off, c)


def assert_equal(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got.float() != want.float()).nonzero()
        raise AssertionError(f"{what}: {int(bad.shape[0])} elements differ, the first at (n, t, ch, y, x) = {bad[0].tolist()}: "
                             f"{float(got.float()[tuple(bad[0])])} against {float(want.float()[tuple(bad[0])])}")


def check_case(backend, device, name, case, dtype=torch.float32):
    """what the stacked launch writes equals roi_warp32 bit for bit, is not all zeros, and is zeros under the far-out rows"""
    want = expected32(case).to(dtype)
    got = launch_stacked(backend, device, case, dtype)
    assert bool(want.any()) and bool(got.any()), f"{name}: a comparison of zeros"
    assert_equal(got, want, f"{name} against roi_warp32")
    for k in case["where"].get("far", []):
        assert not got[k].any(), f"{name}: far-out row {k} did not give zeros"
    return got


def check_f64(backend, device, name, case):
    """|kernel - roi_warp64| <= bound, element by element (fp32 destination)"""
    src = case["src"]
    got = launch_stacked(backend, device, case, torch.float32).double()
    ref = roi_warp64(src, byte_lut(), case["box"], case["warp"], case["out_h"], case["out_w"], case["antialias"])
    b = bound(case["box"], src.shape[2], src.shape[3], case["out_h"], case["out_w"], case["antialias"], byte_lut())
    err = float((got - ref).abs().max())
    print(f"{name}: max |kernel - roi_warp64| = {err:.3e}, bound {b:.3e}")
    assert bool(ref.any()) and err <= b, f"{name}: max |kernel - roi_warp64| = {err:.3e} exceeds the derived bound {b:.3e}"


def source_case(antialias, out_hw=(17, 33)):
    """two clips of three frames told three ways: frames A, A again and a missing one; B, a missing one and C"""
    g = torch.Generator().manual_seed(5)
    a, b, c = (torch.randint(0, 256, (H, W, C), generator=g, dtype=torch.uint8) for _ in range(3))
    fillf = torch.full((H, W, C), FILL, dtype=torch.uint8)
    stacked = torch.stack([torch.stack([a, a, fillf]), torch.stack([b, fillf, c])])
    box = torch.tensor([[3, 2, 50, 37], [10, 8, 40, 30]], dtype=torch.int32)
    warp = torch.cat([draw_affine(1, out_hw[1], 3, 30.0, (0.6, 1.6), 10.0, 0.5, generator=g),
                      torch.tensor([[1.0, 0.0, -2.0, 0.0, 1.0, 1.0]])])
    missing = torch.tensor([[False, False, True], [False, True, False]])
    # the pool: frames in another order, with a padded pixel pitch (9 bytes, channels 1 .. 7) and padded strides
    pitch, c0 = 9, 1
    gp = torch.Generator().manual_seed(6)
    pool = torch.randint(0, 256, (3, H + 1, W + 2, pitch), generator=gp, dtype=torch.uint8)[:, :H, :W]
    for f, fr in enumerate((b, a, c)):
        pool[f, :, :, c0:c0 + C] = fr
    index = torch.tensor([[1, 1, -1], [0, 3, 2]], dtype=torch.int32)
    # the arena: clip 0's frames whole, clip 1's cropped to a rectangle around its box, pixel pitch 7
    rect = (8, 5, 44, 33)                                      # x1, y1, x2, y2 holds clip 1's box
    parts, offs, at = [], {}, 0
    for key, fr in (("a", a), ("b", b[rect[1]:rect[3], rect[0]:rect[2]]), ("c", c[rect[1]:rect[3], rect[0]:rect[2]])):
        at = -(-at // 16) * 16
        offs[key] = at
        parts.append((at, fr.contiguous().view(-1)))
        at += fr.numel()
    arena = torch.randint(0, 256, (-(-at // 4) * 4,), generator=gp, dtype=torch.uint8)
    for o, bts in parts:
        arena[o:o + bts.numel()] = bts
    # a -1 offset, and one that fails the "lies in the arena whole" test by four bytes
    offset = torch.tensor([[offs["a"], offs["a"], -1], [offs["b"], arena.numel() - (rect[3] - rect[1]) * (rect[2] - rect[0]) * C + 4,
                                                         offs["c"]]], dtype=torch.int64)
    hw = torch.tensor([[H, W], [rect[3] - rect[1], rect[2] - rect[0]]], dtype=torch.int32)
    rbox = box.clone()
    rbox[1] -= torch.tensor([rect[0], rect[1], rect[0], rect[1]], dtype=torch.int32)
    return dict(src=stacked, box=box, warp=warp, out_h=out_hw[0], out_w=out_hw[1], antialias=antialias, missing=missing, where={},
                pool=pool, index=index, c0=c0, arena=arena, offset=offset, hw=hw, ragged_box=rbox)


def launch_sources(backend, device, case, dtype=torch.float32):
    """the case through the three entry points: {'stacked', 'pool', 'ragged'} -> what each wrote"""
    n, t = case["index"].shape
    lut, warp = byte_lut().to(device), case["warp"].to(device)
    oh, ow, aa = case["out_h"], case["out_w"], case["antialias"]
    res = {"stacked": launch_stacked(backend, device, case, dtype)}
    pool = case["pool"]
    dev_pool = torch.empty_strided(pool.shape, pool.stride(), dtype=torch.uint8, device=device)
    dev_pool.copy_(pool)
    buf, out, c_off = framed_out(n, t, C, oh, ow, dtype, device)
    backend.roi_resize_pool_warp(dev_pool, case["index"].to(device), lut, FILL, case["box"].to(device), warp, out, aa, c0=case["c0"],
                                 c=C, c_off=c_off)(stream_of(torch.device(device)))
    sync(device)
    res["pool"] = read_framed(buf, out, c_off, C)
    buf, out, c_off = framed_out(n, t, C, oh, ow, dtype, device)
    backend.roi_resize_ragged_warp(case["arena"].to(device), case["offset"].to(device), case["hw"].to(device), lut, FILL,
                                   case["ragged_box"].to(device), warp, out, aa, pitch=C, c_off=c_off, max_hw=(H, W))(stream_of(torch.device(device)))
    sync(device)
    res["ragged"] = read_framed(buf, out, c_off, C)
    return res


def check_sources(backend, device, dtype=torch.float32):
    """the three sources write roi_warp32 of the same clips, so they agree bit for bit"""
    for aa in (False, True):
        case = source_case(aa)
        want = expected32(case).to(dtype)
        assert bool(want[0, 2].any()) and bool(want[1, 1].any()), "a missing frame must not compare as zeros"
        for kind, got in launch_sources(backend, device, case, dtype).items():
            assert_equal(got, want, f"sources aa{int(aa)} {kind} against roi_warp32")


def check_all(backend, device, dtypes=(torch.float32, torch.bfloat16)):
    """every shared check; raises AssertionError at the first that fails"""
    for name, case in all_cases().items():
        for dt in dtypes:
            check_case(backend, device, f"{name} {dt}", case, dt)
    for dt in dtypes:
        check_sources(backend, device, dt)
