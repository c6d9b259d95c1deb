"""Input pipeline step before the hot path: clips cross PCIe as uint8 and are normalised,
transposed and randomly cropped ON the device by one libsfk kernel.

What it replaces (reference dataset/chalearn_dataset.py):
  :41-46   transforms.ToTensor() + Normalize(mean 0.45, std 0.225) per frame  -> a 256-entry fp32 table built here with
           the same two fp32 operations (so every byte maps to the bit pattern the reference produces), applied by
           ``sfk_u8_normalize_crop``;
  :73-85   transforms.RandomCrop(size, padding = size // 10) on the (T, 21, S, S) clip tensor: one (top, left) per clip,
           zeros (of the NORMALISED tensor) outside the frame -> the kernel's per-clip crop offsets;
  train.py:127  the 1.5 GB pageable float32 H2D copy of a 55-clip batch -> a uint8 copy a quarter of that size, staged in
           pinned host memory so that it is an asynchronous DMA.
The reference's ChalearnVideoDataset is untouched: a loader that can hand over its ``img_cat`` frames (HWC uint8, :113)
feeds ``DevicePreprocess``; loaders that deliver float32 batches keep the reference path (ModelManager.prepare_data).
  :131-140 the uniform windows of a test video overlap (stride 4): ``uniform_windows`` restates them as an index table, a test
           video travels as ONE pool of its frames plus that table (the pooled item), and ``FramePool`` uploads every frame
           once and builds the float clips of a batch on the device with ``sfk_u8_pool_gather`` (include/sfk_pool.h).
  :60-71   ``_pad_resize_img`` -- zero-pad the 21-channel crop to a square, cv2.resize(INTER_CUBIC) to S x S: a loader may ship
           the crops at their native, ragged sizes (the raw items) and ``PadResize`` writes the (S, S, 21) uint8 frames on
           the device with one ``sfk_u8_pad_resize_cubic`` launch (include/sfk_resize.h); cv2 is not installed here, the
           arithmetic is pinned to tests/ref_resize.py, parity with cv2 itself unpinned.
  new_feature_test.py:590-661  the v2 part-box loader's crop + /255 + Resize: ``RoiResize`` (one ``sfk_roi_resize`` launch,
           include/sfk_v2.h) from uploaded clips, ``FramePool.roi_gather`` / ``ResidentGestureSet`` (one ``sfk_roi_resize_pool``
           launch, include/sfk_roi_pool.h) from the uncropped frames of the train videos kept in a pool on the device.
torchvision is not installed here, so ToTensor / Normalize / RandomCrop are restated from their documented semantics;
numerically this step is "parity unpinned" against torchvision itself (tests/test_aux_cpu.py pins it to plain torch).
"""
from __future__ import annotations

import bisect
import math

from dataclasses import dataclass
from typing import Optional

import torch

MEAN, STD = 0.45, 0.225          # dataset/chalearn_dataset.py:43-45, all 21 channels


def normalize_lut(mean: float = MEAN, std: float = STD) -> torch.Tensor:
    """float32[256]: ToTensor (uint8 -> float32 / 255) then Normalize ((x - mean) / std), in that order, in fp32."""
    u = torch.arange(256, dtype=torch.uint8)
    x = u.to(torch.float32).div(255)
    return x.sub(torch.tensor(mean, dtype=torch.float32)).div(torch.tensor(std, dtype=torch.float32))


def draw_crop_offsets(n: int, padding: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(n, 2) int32 (top, left), each uniform in [0, 2*padding]: RandomCrop.get_params on the padded (S+2p)^2 image,
    drawn top first, then left, one pair per clip (the crop is applied to the whole (T,21,S,S) tensor, :82-83)."""
    out = torch.empty(n, 2, dtype=torch.int32)
    for i in range(n):
        out[i, 0] = int(torch.randint(0, 2 * padding + 1, (1,), generator=generator))
        out[i, 1] = int(torch.randint(0, 2 * padding + 1, (1,), generator=generator))
    return out


def identity_warp_rows(n: int) -> torch.Tensor:
    """(n, 6) float32 identity rows of the warp table (include/sfk_warp.h): (1, 0, 0, 0, 1, 0)"""
    return torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32).repeat(int(n), 1)


def validate_warp_rows(rows: torch.Tensor) -> torch.Tensor:
    """the host rows of a warp table as contiguous (n, 6) float32, or ValueError: a wrong shape, or an entry that is not a
    finite number (the kernel is memory-safe for any row and writes zeros for such a one; the host refuses it all the same,
    as ``ClipMix.validate`` refuses its rows, because a clip of zeros is never what a loader meant)"""
    rows = torch.as_tensor(rows).detach().to("cpu", torch.float32).contiguous()
    if rows.dim() != 2 or rows.shape[1] != 6:
        raise ValueError(f"warp rows must be (n, 6), got {tuple(rows.shape)}")
    if not bool(torch.isfinite(rows).all()):
        raise ValueError("warp rows: an entry is not finite")
    return rows


def _affine_linear(angle: float, scale: float, shear: float) -> torch.Tensor:
    """float64 (2, 2) L = R(angle) . Sh(shear) . scale: rotation [[cos, -sin], [sin, cos]], x shear [[1, tan], [0, 1]], degrees"""
    a, s = math.radians(float(angle)), math.radians(float(shear))
    rot = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=torch.float64)
    sh = torch.tensor([[1.0, math.tan(s)], [0.0, 1.0]], dtype=torch.float64)
    return rot @ sh * float(scale)


def affine_forward(size: int, padding: int, top: int, left: int, angle: float = 0.0, scale: float = 1.0, shear: float = 0.0,
                   flipped: bool = False) -> torch.Tensor:
    """float64 (2, 3) source -> output map of one clip: p_out = F . L . (p_src - ctr) + ctr - (left - padding, top - padding),
    L = R . Sh . scale about the centre ctr = ((S-1)/2, (S-1)/2), F = diag(-1, 1) when flipped, then RandomCrop's shift"""
    ctr = torch.full((2,), (int(size) - 1) / 2.0, dtype=torch.float64)
    lin = _affine_linear(angle, scale, shear)
    if flipped:
        lin = torch.tensor([[-1.0, 0.0], [0.0, 1.0]], dtype=torch.float64) @ lin
    d = torch.tensor([float(int(left) - int(padding)), float(int(top) - int(padding))], dtype=torch.float64)
    return torch.cat([lin, (ctr - d - lin @ ctr)[:, None]], 1)


def affine_inverse(size: int, padding: int, top: int, left: int, angle: float = 0.0, scale: float = 1.0, shear: float = 0.0,
                   flipped: bool = False) -> torch.Tensor:
    """float64 (2, 3) output -> source map, ``affine_forward``'s inverse written out (no matrix is inverted numerically):
    A = (1 / scale) . Sh(-shear) . R(-angle) . F and p_src = A . (p_out + (left - padding, top - padding) - ctr) + ctr.  With
    angle 0, scale 1, shear 0 and no flip A is exactly the identity and the row exactly (1, 0, left - padding, 0, 1, top -
    padding)."""
    ctr = torch.full((2,), (int(size) - 1) / 2.0, dtype=torch.float64)
    a, s = math.radians(float(angle)), math.radians(float(shear))
    rot_t = torch.tensor([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]], dtype=torch.float64)
    sh_i = torch.tensor([[1.0, -math.tan(s)], [0.0, 1.0]], dtype=torch.float64)
    inv = sh_i @ rot_t * (1.0 / float(scale))
    if flipped:
        inv = inv @ torch.tensor([[-1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    d = torch.tensor([float(int(left) - int(padding)), float(int(top) - int(padding))], dtype=torch.float64)
    return torch.cat([inv, (inv @ (d - ctr) + ctr)[:, None]], 1)


def draw_affine_params(padding: int, degrees: float = 0.0, scale=(1.0, 1.0), shear: float = 0.0, flip: float = 0.0,
                       generator: Optional[torch.Generator] = None) -> tuple:
    """one clip's draws, (top, left, angle, scale, shear, flipped), in the fixed order of ``draw_affine``"""
    top = int(torch.randint(0, 2 * padding + 1, (1,), generator=generator))
    left = int(torch.randint(0, 2 * padding + 1, (1,), generator=generator))
    u = [float(torch.rand(1, dtype=torch.float64, generator=generator)) for _ in range(4)]
    lo, hi = float(scale[0]), float(scale[1])
    return (top, left, -float(degrees) + 2.0 * float(degrees) * u[0], lo + (hi - lo) * u[1],
            -float(shear) + 2.0 * float(shear) * u[2], u[3] < float(flip))


def draw_affine(n: int, size: int, padding: int, degrees: float = 0.0, scale=(1.0, 1.0), shear: float = 0.0, flip: float = 0.0,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(n, 6) float32 rows (a, b, c, d, e, f) for ``sfk_u8_pool_gather_warp`` (include/sfk_warp.h) on S x S frames: the INVERSE
    (output -> source) matrix of a random affine transform about the centre ((S-1)/2, (S-1)/2), formed in float64
    (``affine_inverse``) and rounded once to fp32.  Output pixel (x, y) reads the source at (a x + b y + c, d x + e y + f).
    Composition, source -> output: rotation . shear . scale about the centre (the angle uniform in [-degrees, degrees], the
    isotropic scale uniform in [scale[0], scale[1]], the x shear uniform in [-shear, shear] degrees), an optional horizontal
    flip about the centre (probability ``flip``), then RandomCrop's translation by (padding - left, padding - top).
    Draw order per clip, FIXED and independent of the configuration, so the stream position never depends on which ranges
    are degenerate: (top, left) by the very ``torch.randint(0, 2 * padding + 1, (1,))`` calls ``draw_crop_offsets`` makes,
    then one float64 ``torch.rand(1)`` each for the angle, the scale, the shear and the flip (flipped when u < flip, so 0
    never flips and 1 always does).  With degrees 0, scale (1, 1), shear 0 and flip 0 the row is exactly (1, 0, left - padding,
    0, 1, top - padding): RandomCrop's.
    All 21 channels of a clip are warped as IMAGES -- BGR, U, V, the five flow images and depth alike: the flow is stored as
    colour images and nothing re-orients its vectors under a rotation or a flip.  ``flip`` defaults to 0 because left and right
    hands differ.  Stated in plain torch: torchvision is not installed here, parity with its RandomAffine is unpinned."""
    lo, hi = float(scale[0]), float(scale[1])
    assert n > 0 and size > 0 and padding >= 0 and degrees >= 0 and 0 < lo <= hi and 0 <= shear < 90 and 0 <= flip <= 1
    out = torch.empty(n, 6, dtype=torch.float32)
    for i in range(n):
        p = draw_affine_params(padding, degrees, (lo, hi), shear, flip, generator)
        out[i] = affine_inverse(size, padding, *p).reshape(6).to(torch.float32)
    return out


def draw_color_jitter(n: int, brightness: float = 0.5, contrast: float = 0.3, saturation: float = 0.2, hue: float = 0.1,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(n, 8) float32 rows (order[4], b, c, s, h) for ``sfk_color_jitter``: per clip the draws of torchvision's
    ColorJitter.get_params in its order -- ``torch.randperm(4)``, then one ``torch.empty(1).uniform_(lo, hi)`` each for
    brightness, contrast and saturation from [max(0, 1 - v), 1 + v] and for hue from [-v, v] (the defaults are
    dataset/chalearn_dataset.py:48-50's).  An op whose range is 0 takes no draw and its slot of the order becomes -1, as
    torchvision skips an op whose factor is None; its factor column holds the identity."""
    vals = (float(brightness), float(contrast), float(saturation), float(hue))
    assert all(v >= 0 for v in vals) and vals[3] <= 0.5, vals
    out = torch.empty(n, 8, dtype=torch.float32)
    for i in range(n):
        order = torch.randperm(4, generator=generator).to(torch.float32)
        for op, v in enumerate(vals):
            lo, hi = (-v, v) if op == 3 else (max(0.0, 1.0 - v), 1.0 + v)
            if v == 0:
                order[order == op] = -1.0
                out[i, 4 + op] = 0.0 if op == 3 else 1.0
            else:
                out[i, 4 + op] = float(torch.empty(1).uniform_(lo, hi, generator=generator))
        out[i, :4] = order
    return out


def h2d(t: torch.Tensor, device) -> torch.Tensor:
    """through pinned host memory: the uint8 batch crosses PCIe as an asynchronous DMA behind the previous step's
    kernels (from pageable memory `non_blocking=True` is a synchronous staged copy)"""
    if t.device.type == "cpu" and torch.device(device).type == "cuda" and not t.is_pinned():
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def stream_of(device) -> int:
    """the handle of the current stream of a cuda device; 0 (the emulator backends ignore it) for any other"""
    return torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0


def hip_backend(backend=None):
    """backend, or the library's own when None"""
    if backend is None:
        from ._lib import HipBackend
        backend = HipBackend()                  # raises when libsfk.so is missing: no CPU path
    return backend


class ColorJitter:
    """torchvision's ColorJitter (the reference's train-time colour augmentation, dataset/chalearn_dataset.py:48-50) on the
    three colour planes of a float clip batch (N, T, C, H, W) that already lives on the device, IN PLACE, by
    ``sfk_color_jitter`` (include/sfk_aug.h): two launches on the current stream, one parameter row per clip
    (``draw_color_jitter``).  A stored value s stands for the image value s*std + mean; bgr tells the plane order.
    torchvision is not installed here: the semantics are pinned to plain torch (tests/ref_jitter.py), torchvision itself
    unpinned."""

    def __init__(self, device="cuda", backend=None):
        self.be, self.device = hip_backend(backend), torch.device(device)
        self._ws = {}                           # (n, t, h, w) -> the float32 workspace of that geometry

    def workspace(self, n: int, t: int, h: int, w: int) -> torch.Tensor:
        key = (n, t, h, w)
        if key not in self._ws:
            nbytes = self.be.color_jitter_workspace_bytes(n, t, h, w)
            self._ws[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        return self._ws[key]

    def __call__(self, clip: torch.Tensor, params: torch.Tensor, c_off: int = 0, bgr: bool = False, mean: float = 0.0,
                 std: float = 1.0) -> torch.Tensor:
        assert clip.dim() == 5 and clip.stride(4) == 1 and clip.device.type == self.device.type
        n, t, _, h, w = clip.shape
        params = h2d(params.to(torch.float32), self.device).contiguous()
        assert tuple(params.shape) == (n, 8), tuple(params.shape)
        stream = stream_of(self.device)
        self.be.color_jitter(clip, params, self.workspace(n, t, h, w), c_off, bgr, mean, std)(stream)
        return clip


def identity_mix_rows(n: int) -> torch.Tensor:
    """(n, 8) float32 identity rows of the mix table (include/sfk_mix.h): {own index, 1, 0, 0, 0, 0, 1, 0}"""
    out = torch.zeros(n, 8, dtype=torch.float32)
    out[:, 0] = torch.arange(n, dtype=torch.float32)
    out[:, 1] = 1.0
    out[:, 6] = 1.0
    return out


def _draw_beta(alpha: float, generator: Optional[torch.Generator]) -> float:
    """one Beta(alpha, alpha) draw as g1 / (g1 + g2) of two Gamma(alpha, 1) draws (float64) from ``generator``"""
    g = torch._standard_gamma(torch.full((2,), float(alpha), dtype=torch.float64), generator=generator)
    s = float(g[0] + g[1])
    return float(g[0]) / s if s > 0 else 0.5


def draw_mix(n: int, h: int, w: int, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
             switch_prob: float = 0.5, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(n, 8) float32 rows {partner, lam, y0, x0, y1, x1, weight, 0} for ``sfk_clip_mix`` / ``sfk_softmax_ce_mix``
    (include/sfk_mix.h) on frames of h x w.  Pairing is the flip i <-> n-1-i (the loader's batch is already shuffled); the
    middle clip of an odd batch pairs with itself and keeps the identity row, without a draw.  One draw per pair, shared by
    both members, in this order: u ~ U[0, 1): u >= prob gives identity rows; when both alphas are > 0, v ~ U[0, 1): v <
    switch_prob chooses CutMix (else whichever alpha is > 0); lam ~ Beta(alpha, alpha).  Mixup: lam as drawn, an empty box,
    weight = lam.  CutMix: lam = 1 and the usual box -- sides int(h sqrt(1 - lam)), int(w sqrt(1 - lam)), centre (cy, cx)
    uniform over the frame (cy first), [c - side // 2, c + side // 2) clipped to the frame -- and weight = 1 - box area /
    (h w) after clipping.  Stated in plain torch: timm is not installed here, parity with timm itself is unpinned."""
    assert n > 0 and h > 0 and w > 0 and mixup_alpha >= 0 and cutmix_alpha >= 0 and 0 <= prob <= 1 and 0 <= switch_prob <= 1
    out = identity_mix_rows(n)
    if mixup_alpha <= 0 and cutmix_alpha <= 0:
        return out
    for i in range(n // 2):
        j = n - 1 - i
        out[i, 0], out[j, 0] = float(j), float(i)
        if float(torch.rand(1, generator=generator)) >= prob:
            continue
        cut = cutmix_alpha > 0 and (mixup_alpha <= 0 or float(torch.rand(1, generator=generator)) < switch_prob)
        lam = _draw_beta(cutmix_alpha if cut else mixup_alpha, generator)
        if cut:
            ratio = math.sqrt(max(0.0, 1.0 - lam))
            ch, cw = int(h * ratio), int(w * ratio)
            cy = int(torch.randint(0, h, (1,), generator=generator))
            cx = int(torch.randint(0, w, (1,), generator=generator))
            y0, y1 = min(max(cy - ch // 2, 0), h), min(max(cy + ch // 2, 0), h)
            x0, x1 = min(max(cx - cw // 2, 0), w), min(max(cx + cw // 2, 0), w)
            row = [1.0, y0, x0, y1, x1, 1.0 - ((y1 - y0) * (x1 - x0)) / float(h * w)]
        else:
            row = [lam, 0, 0, 0, 0, lam]
        out[i, 1:7] = out[j, 1:7] = torch.tensor(row, dtype=torch.float32)
    return out


class ClipMix:
    """Mixup / CutMix of a float clip batch (N, T, C, H, W) that already lives on the device, IN PLACE, by ``sfk_clip_mix``
    (include/sfk_mix.h): one launch on the current stream that reads both members of a pair once and writes both, with no
    second clip.  The object owns ONE device table of ``batch_size`` rows: ``load`` validates a batch's host rows
    (``draw_mix``) and copies them into its first n rows, so the table's address is the same from step to step and a
    captured train step (``TrainStep(..., mix=table)``) follows every new draw."""

    def __init__(self, device="cuda", backend=None, batch_size: int = 1):
        self.be, self.device = hip_backend(backend), torch.device(device)
        self.table = identity_mix_rows(int(batch_size)).to(self.device)

    @staticmethod
    def validate(rows: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """the host rows as contiguous float32, or ValueError: a partner outside [0, n) or not mutual, lam or weight outside
        [0, 1], a box outside the h x w frame"""
        rows = rows.detach().to("cpu", torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != 8:
            raise ValueError(f"mix rows must be (n, 8), got {tuple(rows.shape)}")
        n = rows.shape[0]
        part = rows[:, 0]
        if not bool(((part >= 0) & (part < n) & (part == part.floor())).all()):
            raise ValueError(f"mix rows: a partner is outside [0, {n})")
        pi = part.long()
        if not bool((pi[pi] == torch.arange(n)).all()):
            raise ValueError("mix rows: a partner is not mutual (partner[partner[i]] != i)")
        for name, col in (("lam", 1), ("weight", 6)):
            if not bool(((rows[:, col] >= 0) & (rows[:, col] <= 1)).all()):
                raise ValueError(f"mix rows: a {name} is outside [0, 1]")
        y0, x0, y1, x1 = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
        if not bool(((y0 >= 0) & (x0 >= 0) & (y1 <= h) & (x1 <= w) & (y0 <= h) & (x0 <= w) & (y1 >= 0) & (x1 >= 0)).all()):
            raise ValueError(f"mix rows: a box is outside the {h} x {w} frame")
        return rows

    def load(self, rows: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """validate (n, 8) host rows for frames of h x w, copy them into the first n rows of the table, return that view"""
        rows = self.validate(rows, h, w)
        n = rows.shape[0]
        if n > self.table.shape[0]:
            raise ValueError(f"{n} mix rows for a table of {self.table.shape[0]} (the batch size it was built for)")
        view = self.table[:n]
        view.copy_(h2d(rows, self.device), non_blocking=True)
        return view

    def __call__(self, clip: torch.Tensor, table: torch.Tensor, c_off: int = 0, c: Optional[int] = None) -> torch.Tensor:
        assert clip.dim() == 5 and clip.stride(4) == 1 and clip.device.type == self.device.type
        assert table.dtype == torch.float32 and tuple(table.shape) == (clip.shape[0], 8), tuple(table.shape)
        self.be.clip_mix(clip, table, c_off, c)(stream_of(self.device))
        return clip


class DevicePreprocess:
    """uint8 frames (N, T, S, S, C) -> normalised clip batch (N, T, C, S, S) on the device.  crop (N, 2): RandomCrop's shift,
    by ``sfk_u8_normalize_crop``; warp (N, 6) float32 (``draw_affine``) instead: every clip sampled through its matrix, by ONE
    ``sfk_u8_pool_gather_warp`` launch (include/sfk_warp.h) over the stacked frames, which are a pool that needs no index
    table; the rows are validated on the host first (``validate_warp_rows``).  crop and warp together is a ValueError."""

    def __init__(self, device="cuda", backend=None, out_dtype: torch.dtype = torch.float32):
        self.be, self.device, self.out_dtype = hip_backend(backend), torch.device(device), out_dtype
        self.lut = normalize_lut().to(self.device)

    def __call__(self, frames_u8: torch.Tensor, crop: Optional[torch.Tensor] = None, padding: Optional[int] = None,
                 warp: Optional[torch.Tensor] = None):
        assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 5
        if crop is not None and warp is not None:
            raise ValueError("DevicePreprocess: crop and warp together (a warp row carries RandomCrop's translation itself)")
        n, t, h, w, c = frames_u8.shape
        x = h2d(frames_u8, self.device).contiguous()
        if warp is not None:
            rows = validate_warp_rows(warp)
            assert tuple(rows.shape) == (n, 6), tuple(rows.shape)
            out = torch.empty(n, t, c, h, w, dtype=self.out_dtype, device=self.device)
            self.be.u8_pool_gather_warp(x, None, self.lut, MISSING_BYTE, h2d(rows, self.device), out)(stream_of(self.device))
            return out
        if crop is not None:
            padding = h // 10 if padding is None else padding
            crop = h2d(crop.to(torch.int32), self.device).contiguous()
            assert tuple(crop.shape) == (n, 2)
        out = torch.empty(n, t, c, h, w, dtype=self.out_dtype, device=self.device)
        stream = stream_of(self.device)
        self.be.u8_normalize_crop(x, self.lut, crop, int(padding or 0), out)(stream)
        return out


MISSING_BYTE = 127               # dataset/chalearn_dataset.py:116: every byte of a frame whose file is missing


def uniform_windows(seq_len: int, clip_len: int, stride: int = 4) -> torch.Tensor:
    """(K, T) int32 frame indices of the reference's ``uniform_sampling`` (dataset/chalearn_dataset.py:131-140): a video of at
    most clip_len frames gives ONE window that wraps around (its random_sampling draws randint(0, 0) = 0); a longer one gives
    the windows starting at range(0, seq_len - clip_len, stride) -- the tail of a video may belong to no window, as there."""
    assert seq_len >= 1 and clip_len >= 1 and stride >= 1, (seq_len, clip_len, stride)
    if seq_len <= clip_len:
        return torch.tensor([[i % seq_len for i in range(clip_len)]], dtype=torch.int32)
    starts = torch.arange(0, seq_len - clip_len, stride, dtype=torch.int32)
    return starts[:, None] + torch.arange(clip_len, dtype=torch.int32)[None, :]


def pool_key(key: str) -> str:
    return key + "_pool"


def _read_referenced(windows: torch.Tensor, read) -> tuple:
    """(the frames some window references that exist, each read ONCE, in ascending order; windows (K, T) int32 renumbered
    densely into that list, -1 for a missing frame); a video with no existing frame is a ValueError"""
    windows = torch.as_tensor(windows, dtype=torch.int32)
    remap, frames = {}, []
    for i in sorted(set(windows.flatten().tolist())):
        f = read(i)
        if f is None:
            remap[i] = -1
        else:
            remap[i] = len(frames)
            frames.append(f)
    if not frames:
        raise ValueError("a pooled video needs at least one frame that exists")
    local = torch.tensor([[remap[i] for i in row] for row in windows.tolist()], dtype=torch.int32)
    return frames, local


def make_pooled_item(key: str, windows: torch.Tensor, label, read) -> dict:
    """The pooled item of one test video: {'<key>_pool': (F, S, S, P) uint8 HWC, 'windows': (K, T) int32, 'label'}.
    windows holds indices into the VIDEO; read(i) returns frame i as (S, S, P) uint8, or None when it is missing, and is
    called once per frame that some window references.  Only those frames that exist enter the pool, renumbered densely
    in ascending order; a missing frame becomes -1 in 'windows'."""
    frames, local = _read_referenced(windows, read)
    return {pool_key(key): torch.stack([torch.as_tensor(f) for f in frames]), "windows": local, "label": label}


def unpool_item(item: dict) -> list:
    """A pooled item as the list of clip dicts it stands for, [{'<key>_u8': (T, S, S, P) uint8, 'label'}] -- the uint8
    transport's test item -- with every missing frame (-1) materialised as bytes of 127."""
    pk = next(k for k in item if k.endswith("_pool"))
    pool, windows = item[pk], item["windows"]
    ext = torch.cat([pool, torch.full_like(pool[:1], MISSING_BYTE)])       # the last entry stands for -1
    idx = windows.long()
    if int(idx.min()) < -1 or int(idx.max()) >= pool.shape[0]:
        raise ValueError(f"window index outside [-1, {pool.shape[0]})")
    return [{pk[:-len("_pool")] + "_u8": ext[row], "label": item["label"]} for row in idx]


def _persistent_table(tables: dict, name: str, host: torch.Tensor, device) -> torch.Tensor:
    """host table -> its view of the persistent device buffer tables[name], written on the current stream.  The buffer is
    sized at first use and grows to the largest table seen, so equal-shaped batches get the SAME address (a smaller one the
    same base); the copy is ordered behind every launch already enqueued that reads the old contents."""
    buf = tables.get(name)
    if buf is None or buf.numel() < host.numel():
        buf = tables[name] = torch.empty(host.numel(), dtype=host.dtype, device=device)
    view = buf[:host.numel()].view(host.shape)
    src = host
    if src.device.type == "cpu" and device.type == "cuda" and not src.is_pinned():
        src = src.pin_memory()
    view.copy_(src, non_blocking=True)
    return view


def _roi_tables(who: str, n: int, size: int, box, crop, padding, warp) -> tuple:
    """what ``RoiResize`` and the two ``roi_gather``s (who: the caller a ValueError names) take per batch of n clips, as host
    tensors: (box (n, 4) int32, crop (n, 2) int32 | None, pad, warp (n, 6) float32 validated | None); pad is RandomCrop's
    padding, size // 10 unless given, and 0 without a crop.  Where each is uploaded is the caller's."""
    if crop is not None and warp is not None:
        raise ValueError(f"{who}: crop and warp together (a warp row carries RandomCrop's translation itself)")
    box = torch.as_tensor(box).to(torch.int32).contiguous()
    assert tuple(box.shape) == (n, 4), tuple(box.shape)
    pad = 0
    if crop is not None:
        crop = torch.as_tensor(crop).to(torch.int32).contiguous()
        assert tuple(crop.shape) == (n, 2), tuple(crop.shape)
        pad = size // 10 if padding is None else int(padding)
    if warp is not None:
        warp = validate_warp_rows(warp)
        assert tuple(warp.shape) == (n, 6), tuple(warp.shape)
    return box, crop, pad, warp


class FramePool:
    """The device side of the pooled items: an arena of uint8 HWC frames (capacity, S, S, P) on the device, grown on demand.

    ``add`` uploads the frames of one video ONCE, through pinned memory, into a free run of arena slots and returns the first
    slot (its base); ``rows`` turns the video's window table into arena slots; ``gather`` builds the (N, T, c, S, S) float
    clips of any mix of rows with one ``sfk_u8_pool_gather`` launch; ``release`` returns a video's slots once its last window
    has been gathered.  A video whose windows straddle two batches simply stays in the arena until then.  Every copy and
    launch goes on the current stream, so a slot is never overwritten before the gather that read it has run.
    ``bytes_uploaded`` counts the frame bytes sent host to device.
    capacity: a FIXED number of arena slots -- the arena is allocated once, at the first ``add``, and never grows or moves
    (a video that finds no room is a RuntimeError; ``fits`` asks beforehand); ``gather`` with a crop table builds the
    RandomCrop-ped train clips with ``sfk_u8_pool_gather_crop`` (include/sfk_resident.h).  ``ResidentTrainSet`` uses both.
    ``roi_gather`` is ``RoiResize`` over the pool's frames: the part-box crop + /255 + bilinear resize of the v2 loader from a
    table of arena slots, by ONE ``sfk_roi_resize_pool`` launch (include/sfk_roi_pool.h); ``ResidentGestureSet`` uses it."""

    def __init__(self, device="cuda", backend=None, fill: int = MISSING_BYTE, capacity: Optional[int] = None):
        self.be, self.device, self.fill = hip_backend(backend), torch.device(device), int(fill)
        self.lut = normalize_lut().to(self.device)
        self.arena: Optional[torch.Tensor] = None
        self.live = {}                          # base -> frames of that video
        self.bytes_uploaded = 0
        self._resize = {}                       # (size, channels) -> the PadResize of add_raw
        self._byte_lut = None                   # roi_gather's table, made at its first call
        self._tables = {}                       # persistent device tables: clip's 'index' / 'crop' (int32), gather's 'warp' and roi_gather's 'roi_warp' (float32) -> flat buffer
        self.capacity = None if capacity is None else int(capacity)
        if self.capacity is not None and self.capacity <= 0:
            raise ValueError(f"FramePool: capacity {capacity} frames")

    @staticmethod
    def check_windows(windows: torch.Tensor, frames: int) -> None:
        """every index is -1 (a missing frame) or inside its video's pool; anything else is a ValueError"""
        w = torch.as_tensor(windows)
        if w.numel() and (int(w.min()) < -1 or int(w.max()) >= frames):
            raise ValueError(f"window index outside its video's pool: [{int(w.min())}, {int(w.max())}] against {frames} frames")

    def _place(self, f: int) -> Optional[int]:
        """the first free run of f slots (first fit over the gaps between the live videos), or None"""
        at = 0
        for base in sorted(self.live):
            if base - at >= f:
                return at
            at = base + self.live[base]
        return at if self.arena is not None and self.arena.shape[0] - at >= f else None

    def _grow(self, f: int, frame_shape: tuple) -> None:
        used = max((b + n for b, n in self.live.items()), default=0)
        cap = max(used + f, 2 * (0 if self.arena is None else self.arena.shape[0]))
        new = torch.empty((cap,) + tuple(frame_shape), dtype=torch.uint8, device=self.device)
        for b, n in self.live.items():          # device to device, on the current stream: not an upload
            new[b:b + n].copy_(self.arena[b:b + n], non_blocking=True)
        self.arena = new

    def _reserve(self, f: int, frame_shape: tuple) -> int:
        """the base of a free run of f arena slots of frame_shape (the arena grows, or starts over in a new shape when empty)"""
        if self.arena is not None and tuple(self.arena.shape[1:]) != tuple(frame_shape):
            if self.live or self.capacity is not None:
                raise ValueError(f"frames of {tuple(frame_shape)} in a pool of {tuple(self.arena.shape[1:])}")
            self.arena = None
        if self.capacity is not None:           # a fixed arena: allocated once, never grown, never moved
            if self.arena is None and f <= self.capacity:
                self.arena = torch.empty((self.capacity,) + tuple(frame_shape), dtype=torch.uint8, device=self.device)
            base = self._place(f)
            if base is None:
                raise RuntimeError(f"FramePool: no room for {f} more frames in its fixed capacity of {self.capacity} "
                                   f"({sum(self.live.values())} in use)")
            return base
        base = self._place(f)
        if base is None:
            self._grow(f, frame_shape)
            base = self._place(f)
        return base

    def fits(self, f: int) -> bool:
        """would ``add`` of f frames find room?  (a pool without a capacity grows: always)"""
        if self.capacity is None:
            return True
        if self.arena is None:
            return 0 < int(f) <= self.capacity
        return self._place(int(f)) is not None

    def add(self, video_frames: torch.Tensor, windows: Optional[torch.Tensor] = None) -> int:
        """upload (F, S, S, P) uint8 frames; windows, when given, is checked against F BEFORE anything is uploaded"""
        assert video_frames.dtype == torch.uint8 and video_frames.dim() == 4 and video_frames.shape[0] > 0
        f = int(video_frames.shape[0])
        if windows is not None:
            self.check_windows(windows, f)
        base = self._reserve(f, tuple(video_frames.shape[1:]))
        src = video_frames.contiguous()
        if src.device.type == "cpu" and self.device.type == "cuda" and not src.is_pinned():
            src = src.pin_memory()
        self.arena[base:base + f].copy_(src, non_blocking=True)
        self.live[base] = f
        self.bytes_uploaded += src.numel()
        return base

    def add_raw(self, raw_bytes: torch.Tensor, hw: torch.Tensor, size: int, windows: Optional[torch.Tensor] = None,
                channels: int = 21) -> int:
        """a raw pooled video: its F frames at their native sizes, (h, w, channels) HWC bytes end to end in raw_bytes with
        hw (F, 2) -- upload the BYTES once, reserve F arena slots of (size, size, channels) and let ``PadResize`` write the
        padded, cubic-resized frames straight into them.  windows and the table are checked BEFORE anything is uploaded;
        ``bytes_uploaded`` counts the raw bytes."""
        hw = torch.as_tensor(hw, dtype=torch.int32)
        assert hw.dim() == 2 and hw.shape[1] == 2 and hw.shape[0] > 0
        f = int(hw.shape[0])
        if windows is not None:
            self.check_windows(windows, f)
        key = (int(size), int(channels))
        if key not in self._resize:
            self._resize[key] = PadResize(size, self.device, self.be, fill=self.fill, channels=channels)
        pr = self._resize[key]
        offset = raw_offsets(hw, channels)
        pr.check_table(int(raw_bytes.numel()), offset, hw)
        base = self._reserve(f, (int(size), int(size), int(channels)))
        pr(raw_bytes, offset, hw, out=self.arena[base:base + f])
        self.live[base] = f
        self.bytes_uploaded += int(raw_bytes.numel())
        return base

    def rows(self, base: int, windows: torch.Tensor) -> torch.Tensor:
        """(K, T) int32 arena slots of a video's windows (-1 stays -1)"""
        self.check_windows(windows, self.live[base])
        w = torch.as_tensor(windows, dtype=torch.int32)
        return torch.where(w < 0, w, w + base)

    def release(self, base: int) -> None:
        del self.live[base]

    def _checked_rows(self, index_rows: torch.Tensor, who: str = "gather") -> torch.Tensor:
        """the (N, T) int32 table of ``gather`` / ``clip`` (who: the caller the ValueError names): every entry -1 or a slot of a
        video that is in the pool"""
        idx = torch.as_tensor(index_rows, dtype=torch.int32).contiguous()
        assert idx.dim() == 2 and idx.numel() > 0 and self.arena is not None
        ok = torch.zeros(self.arena.shape[0] + 1, dtype=torch.bool)      # the last entry stands for -1
        ok[-1] = True
        for b, n in self.live.items():
            ok[b:b + n] = True
        if int(idx.min()) < -1 or int(idx.max()) >= self.arena.shape[0] or not bool(ok[idx.long()].all()):
            raise ValueError(f"{who}: an index is neither -1 nor a slot of a video that is in the pool")
        return idx

    def _table(self, name: str, host: torch.Tensor) -> torch.Tensor:
        """host table (int32; float32 for 'warp' and 'roi_warp') -> its view of the pool's persistent device buffer `name`"""
        return _persistent_table(self._tables, name, host, self.device)

    def clip(self, index_rows: torch.Tensor, channels, crop: Optional[torch.Tensor] = None,
             padding: Optional[int] = None) -> list:
        """(N, T) arena slots (or -1) -> one ``PoolClip`` per (c0, c) range of channels: the clips ``gather`` would write,
        handed to the stems as the arena and the two tables instead (include/sfk_u8stem_pool.h, MODEL.POOL_STEM).  The table
        is checked as ``gather`` checks it; nothing is launched.  The slots must stay live until the launches that read the
        clips have been enqueued on this stream, and the next ``clip`` call overwrites the tables these clips hold."""
        idx = self._checked_rows(index_rows, "clip")
        h = self.arena.shape[1]
        if crop is not None:
            crop = torch.as_tensor(crop).to(torch.int32).contiguous()
            assert tuple(crop.shape) == (idx.shape[0], 2), tuple(crop.shape)
            crop = self._table("crop", crop)
        padding = h // 10 if padding is None else int(padding)
        index = self._table("index", idx)
        return [PoolClip(self.arena, index, int(c0), int(c), crop, padding, self.lut, self.fill) for c0, c in channels]

    def gather(self, index_rows: torch.Tensor, out_dtype: torch.dtype = torch.float32, c0: int = 0,
               c: Optional[int] = None, crop: Optional[torch.Tensor] = None, padding: Optional[int] = None,
               warp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, T) arena slots (or -1) -> the (N, T, c, S, S) clips DevicePreprocess would write from the materialised frames;
        crop (N, 2) int32 (top, left): with that RandomCrop (padding defaults to S // 10, as DevicePreprocess's), by ONE
        ``sfk_u8_pool_gather_crop`` launch instead of the ``sfk_u8_pool_gather`` one; warp (N, 6) float32 (``draw_affine``)
        instead of crop: every clip sampled through its matrix, by ONE ``sfk_u8_pool_gather_warp`` launch (include/sfk_warp.h),
        the validated rows written into the pool's persistent 'warp' table"""
        idx = self._checked_rows(index_rows)
        _, h, w, p = self.arena.shape
        c = p - c0 if c is None else c
        if crop is not None and warp is not None:
            raise ValueError("gather: crop and warp together (a warp row carries RandomCrop's translation itself)")
        out = torch.empty(idx.shape[0], idx.shape[1], c, h, w, dtype=out_dtype, device=self.device)
        stream = stream_of(self.device)
        if warp is not None:
            rows = validate_warp_rows(warp)
            assert tuple(rows.shape) == (idx.shape[0], 6), tuple(rows.shape)
            self.be.u8_pool_gather_warp(self.arena, h2d(idx, self.device), self.lut, self.fill, self._table("warp", rows), out,
                                        c0, c)(stream)
            return out
        if crop is not None:
            crop = torch.as_tensor(crop).to(torch.int32).contiguous()
            assert tuple(crop.shape) == (idx.shape[0], 2), tuple(crop.shape)
            padding = h // 10 if padding is None else int(padding)
            self.be.u8_pool_gather_crop(self.arena, h2d(idx, self.device), self.lut, self.fill, h2d(crop, self.device), padding,
                                        out, c0, c)(stream)
            return out
        self.be.u8_pool_gather(self.arena, h2d(idx, self.device), self.lut, self.fill, out, c0, c)(stream)
        return out

    def roi_gather(self, index_rows: torch.Tensor, box: torch.Tensor, size: int, out_dtype: torch.dtype = torch.float32,
                   antialias: bool = True, crop: Optional[torch.Tensor] = None, padding: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, warp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, T) arena slots (or -1) and boxes (N, 4) = (x1, y1, x2, y2) -> the (N, T, c, size, size) clips ``RoiResize``
        would write from the materialised frames (a -1 frame materialised as bytes of ``fill``), through ``byte_lut()``; crop
        (N, 2) int32 (top, left): with RandomCrop(size, padding) after the resize (padding defaults to size // 10, as
        RoiResize's).  The same liveness check of every index as ``gather``; ONE ``sfk_roi_resize_pool`` launch on the
        current stream; the H2D of the index, box and crop tables only.  warp (N, 6) float32 (``draw_affine``) instead of
        crop: ONE ``sfk_roi_resize_pool_warp`` launch (include/sfk_roi_warp.h) instead, the validated rows written into the
        pool's persistent 'roi_warp' table; crop and warp together is a ValueError."""
        size = int(size)
        box, crop, pad, warp = _roi_tables("roi_gather", len(index_rows), size, box, crop, padding, warp)
        idx = self._checked_rows(index_rows, "roi_gather")
        if self._byte_lut is None:
            self._byte_lut = byte_lut().to(self.device)
        if out is None:
            out = torch.empty(idx.shape[0], idx.shape[1], self.arena.shape[3], size, size, dtype=out_dtype, device=self.device)
        stream = stream_of(self.device)
        if warp is not None:
            self.be.roi_resize_pool_warp(self.arena, h2d(idx, self.device), self._byte_lut, self.fill, h2d(box, self.device),
                                         self._table("roi_warp", warp), out, bool(antialias))(stream)
            return out
        self.be.roi_resize_pool(self.arena, h2d(idx, self.device), self._byte_lut, self.fill, h2d(box, self.device), out,
                                bool(antialias), None if crop is None else h2d(crop, self.device), pad)(stream)
        return out


class BoxArena:
    """A byte arena next to ``FramePool`` for frames that differ in shape from video to video: ONE uint8 tensor of
    capacity_bytes (rounded down to a multiple of 16), allocated at the first ``add`` and never grown or moved.

    ``add`` uploads the (L, h, w, P) frames of one block ONCE, through pinned memory, to the first free run of bytes that
    starts at a multiple of 16 (first fit over the gaps between the live blocks) and returns that byte offset (its base);
    ``offsets`` turns the block's window table into the byte offset of every frame; ``roi_gather`` builds the
    (N, T, P, size, size) clips ``RoiResize`` would write from the frames behind any mix of offsets, each clip with its own
    stored rectangle, by ONE ``sfk_roi_resize_ragged`` launch (include/sfk_roi_ragged.h); ``release`` returns a block's bytes.
    Every copy and launch goes on the current stream, so a byte is never overwritten before the gather that read it has run.
    ``bytes_uploaded`` counts the frame bytes sent host to device.  ``ResidentGestureSet(store='box')`` uses it."""
    ALIGN = 16

    def __init__(self, capacity_bytes: int, device="cuda", backend=None, fill: int = MISSING_BYTE):
        self.be, self.device, self.fill = hip_backend(backend), torch.device(device), int(fill)
        self.capacity = int(capacity_bytes) // self.ALIGN * self.ALIGN
        if self.capacity <= 0:
            raise ValueError(f"BoxArena: capacity {capacity_bytes} bytes")
        self.arena: Optional[torch.Tensor] = None
        self.live = {}                          # base -> (L, h, w, P) of that block
        self.pitch: Optional[int] = None        # P: that of the first block, and of every block after it
        self.bytes_uploaded = 0
        self._byte_lut = None                   # roi_gather's table, made at its first call
        self._tables = {}                       # persistent device tables: roi_gather's 'roi_warp' (float32) -> flat buffer

    @classmethod
    def _span(cls, shape) -> int:
        """the bytes a block of that shape holds in the arena: its own, rounded up to the alignment"""
        l, h, w, p = shape
        return -(-(l * h * w * p) // cls.ALIGN) * cls.ALIGN

    def _place(self, nbytes: int) -> Optional[int]:
        at = 0
        for base in sorted(self.live):
            if base - at >= nbytes:
                return at
            at = base + self._span(self.live[base])
        return at if self.capacity - at >= nbytes else None

    def fits(self, nbytes: int) -> bool:
        """would ``add`` of a block of nbytes find room?"""
        return int(nbytes) > 0 and self._place(-(-int(nbytes) // self.ALIGN) * self.ALIGN) is not None

    def add(self, frames: torch.Tensor) -> int:
        """upload (L, h, w, P) uint8 frames; the byte offset of the first"""
        assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.numel() > 0, (frames.dtype, tuple(frames.shape))
        shape = tuple(int(v) for v in frames.shape)
        if self.pitch is not None and shape[3] != self.pitch:
            raise ValueError(f"BoxArena: frames of {shape[3]} bytes a pixel in an arena of {self.pitch}")
        base = self._place(self._span(shape))
        if base is None:
            raise RuntimeError(f"BoxArena: no room for {frames.numel()} more bytes in its fixed capacity of {self.capacity} "
                               f"({sum(self._span(v) for v in self.live.values())} in use)")
        if self.arena is None:
            self.arena = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        src = frames.contiguous().view(-1)
        if src.device.type == "cpu" and self.device.type == "cuda" and not src.is_pinned():
            src = src.pin_memory()
        self.arena[base:base + src.numel()].copy_(src, non_blocking=True)
        self.live[base], self.pitch = shape, shape[3]
        self.bytes_uploaded += src.numel()
        return base

    def offsets(self, base: int, windows: torch.Tensor) -> torch.Tensor:
        """(K, T) int64 byte offsets of a block's windows (-1 stays -1)"""
        l, h, w, p = self.live[base]
        FramePool.check_windows(windows, l)
        win = torch.as_tensor(windows, dtype=torch.int64)
        return torch.where(win < 0, win, base + win * (h * w * p))

    def release(self, base: int) -> None:
        del self.live[base]

    def _check_table(self, off: torch.Tensor, hw: torch.Tensor, box: torch.Tensor) -> None:
        """every offset is -1 or the start of a frame of a live block whose (h, w) is its clip's hw row; every box lies in
        its clip's rectangle (one that does not would silently differ from whole-frame storage)"""
        bases = sorted(self.live)
        for n in range(off.shape[0]):
            h, w = (int(v) for v in hw[n])
            x1, y1, x2, y2 = (int(v) for v in box[n])
            if not (0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h):
                raise ValueError(f"roi_gather: box {(x1, y1, x2, y2)} of clip {n} is not inside its {w}x{h} rectangle")
            for o in set(off[n].tolist()):
                if o == -1:
                    continue
                k = bisect.bisect_right(bases, o) - 1
                ok = k >= 0
                if ok:
                    l, bh, bw, p = self.live[bases[k]]
                    rel, fb = o - bases[k], bh * bw * p
                    ok = (bh, bw) == (h, w) and rel % fb == 0 and rel // fb < l
                if not ok:
                    raise ValueError(f"roi_gather: offset {o} of clip {n} is neither -1 nor the start of a {w}x{h} frame of a "
                                     "block that is in the arena")

    def roi_gather(self, offset_rows: torch.Tensor, hw: torch.Tensor, box: torch.Tensor, size: int,
                   out_dtype: torch.dtype = torch.float32, antialias: bool = True, crop: Optional[torch.Tensor] = None,
                   padding: Optional[int] = None, out: Optional[torch.Tensor] = None,
                   warp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, T) byte offsets (or -1), the clips' stored rectangles hw (N, 2) = (h_n, w_n) and their boxes (N, 4) =
        (x1, y1, x2, y2) IN those rectangles -> the (N, T, P, size, size) clips ``RoiResize`` would write from those frames (a
        -1 frame as bytes of ``fill``), through ``byte_lut()``; crop and padding as ``FramePool.roi_gather``'s.  The host
        checks of ``_check_table`` first; then ONE ``sfk_roi_resize_ragged`` launch on the current stream, its tile sized from
        the largest rectangle of THIS batch, and the H2D of the offset, hw, box and crop tables only.  warp (N, 6) float32
        (``draw_affine``) instead of crop: ONE ``sfk_roi_resize_ragged_warp`` launch (include/sfk_roi_warp.h) instead, the
        validated rows written into the arena's persistent warp table; crop and warp together is a ValueError.  The matrix
        lives in the coordinates of the RESIZED image, so the rectangle's origin, which translates the box, does not touch it."""
        size = int(size)
        box, crop, pad, warp = _roi_tables("roi_gather", len(offset_rows), size, box, crop, padding, warp)
        off = torch.as_tensor(offset_rows, dtype=torch.int64).contiguous()
        assert off.dim() == 2 and off.numel() > 0 and self.arena is not None
        n, pitch = off.shape[0], self.pitch
        hw = torch.as_tensor(hw).to(torch.int32).contiguous()
        assert tuple(hw.shape) == (n, 2), tuple(hw.shape)
        self._check_table(off, hw, box)
        if self._byte_lut is None:
            self._byte_lut = byte_lut().to(self.device)
        if out is None:
            out = torch.empty(n, off.shape[1], pitch, size, size, dtype=out_dtype, device=self.device)
        stream, max_hw = stream_of(self.device), (int(hw[:, 0].max()), int(hw[:, 1].max()))
        if warp is not None:
            self.be.roi_resize_ragged_warp(self.arena, h2d(off, self.device), h2d(hw, self.device), self._byte_lut, self.fill,
                                           h2d(box, self.device), _persistent_table(self._tables, "roi_warp", warp, self.device),
                                           out, bool(antialias), pitch=pitch, max_hw=max_hw)(stream)
            return out
        self.be.roi_resize_ragged(self.arena, h2d(off, self.device), h2d(hw, self.device), self._byte_lut, self.fill,
                                  h2d(box, self.device), out, bool(antialias), None if crop is None else h2d(crop, self.device),
                                  pad, pitch=pitch, max_hw=max_hw)(stream)
        return out


def raw_key(key: str) -> str:
    return key + "_raw"


def rawpool_key(key: str) -> str:
    return key + "_rawpool"


def raw_offsets(hw: torch.Tensor, channels: int) -> torch.Tensor:
    """int64 first byte of every frame of hw (..., 2) = (h, w) when the frames' HWC bytes lie end to end in table order; a
    frame with a non-positive side has no bytes"""
    hw = torch.as_tensor(hw).to(torch.int64)
    nbytes = (hw[..., 0].clamp(min=0) * hw[..., 1].clamp(min=0) * int(channels)).flatten()
    return (torch.cumsum(nbytes, 0) - nbytes).reshape(hw.shape[:-1])


def pack_raw_frames(frames) -> tuple:
    """[(h, w, c) uint8 HWC frame, or None for a missing one] -> (their bytes end to end, 1-D uint8; hw (F, 2) int32 with
    (0, 0) for a missing frame)"""
    parts, hw = [], []
    for f in frames:
        if f is None:
            hw.append((0, 0))
            continue
        f = torch.as_tensor(f)
        assert f.dtype == torch.uint8 and f.dim() == 3, (f.dtype, tuple(f.shape))
        parts.append(f.contiguous().reshape(-1))
        hw.append((int(f.shape[0]), int(f.shape[1])))
    raw = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8)
    return raw, torch.tensor(hw, dtype=torch.int32).reshape(-1, 2)


def make_raw_item(key: str, frames, label) -> dict:
    """The raw train item of one clip: {'<key>_raw': 1-D uint8, 'raw_hw': (T, 2) int32, 'label'} from its T frames (None: a
    missing frame, (0, 0) in raw_hw, which PadResize fills with 127)."""
    raw, hw = pack_raw_frames(frames)
    return {raw_key(key): raw, "raw_hw": hw, "label": label}


def make_raw_pooled_item(key: str, windows: torch.Tensor, label, read) -> dict:
    """``make_pooled_item`` for frames at their native sizes: {'<key>_rawpool': 1-D uint8, 'raw_hw': (F, 2) int32, 'windows':
    (K, T) int32, 'label'}.  read(i) returns frame i as (h, w, c) uint8 HWC, or None when it is missing, once per frame that
    some window references; only the frames that exist are kept, renumbered densely, a missing one is -1 in 'windows'."""
    frames, local = _read_referenced(windows, read)
    raw, hw = pack_raw_frames(frames)
    return {rawpool_key(key): raw, "raw_hw": hw, "windows": local, "label": label}


def collate_raw(items):
    """``default_collate`` for a list of item dicts whose '<key>_raw' entries are ragged: those byte buffers are concatenated
    into ONE 1-D uint8 tensor, in item order, and 'raw_offset' (N, T) int64 holds the first byte of every frame in it (a
    missing frame has no bytes); 'raw_hw' and everything else is collated as default_collate does.  Items without a raw
    entry are left to default_collate."""
    from torch.utils.data.dataloader import default_collate
    if not (isinstance(items[0], dict) and any(k.endswith("_raw") for k in items[0])):
        return default_collate(items)
    rk = next(k for k in items[0] if k.endswith("_raw"))
    out = default_collate([{k: v for k, v in it.items() if k != rk} for it in items])
    bufs = [torch.as_tensor(it[rk]).reshape(-1) for it in items]
    hw = out["raw_hw"]
    per_frame = hw[..., 0].clamp(min=0).to(torch.int64) * hw[..., 1].clamp(min=0).to(torch.int64)
    pixels = per_frame.sum(dim=tuple(range(1, per_frame.dim())))
    starts, at = [], 0
    for it, b, px in zip(items, bufs, pixels.tolist()):
        if px == 0 or b.numel() % px:
            if b.numel():
                raise ValueError(f"{rk}: {b.numel()} bytes for {px} pixels")
            c = 1
        else:
            c = b.numel() // px
        starts.append(raw_offsets(torch.as_tensor(it["raw_hw"]), c) + at)
        at += b.numel()
    out[rk] = torch.cat(bufs)
    out["raw_offset"] = torch.stack(starts)
    return out


class PadResize:
    """The reference's ``_pad_resize_img`` (dataset/chalearn_dataset.py:60-71) on the device: crops at their native sizes, HWC
    bytes in one 1-D uint8 buffer with a table of byte offsets and (h, w) pairs, -> the (F, S, S, c) uint8 frames every
    consumer of the uint8 transport reads, by ONE ``sfk_u8_pad_resize_cubic`` launch (include/sfk_resize.h).  The table is
    validated on the host BEFORE anything is uploaded (a span outside the buffer or a negative size is a ValueError; a
    (0, 0) entry is a missing frame and becomes bytes of ``fill``), max_side comes from the table, and bytes and table
    cross through pinned memory.  The arithmetic is integer and pinned to tests/ref_resize.py; cv2 is not installed here,
    parity with cv2.resize(INTER_CUBIC) itself is unpinned.  ``bytes_uploaded`` counts the raw bytes sent."""

    def __init__(self, size: int, device="cuda", backend=None, fill: int = MISSING_BYTE, channels: int = 21):
        self.be, self.device = hip_backend(backend), torch.device(device)
        self.size, self.fill, self.channels = int(size), int(fill), int(channels)
        assert self.size > 0 and 0 <= self.fill <= 255 and self.channels > 0
        self.bytes_uploaded = 0

    def check_table(self, nbytes: int, offset: torch.Tensor, hw: torch.Tensor) -> int:
        """ValueError for a table the kernel would answer with fill bytes although a frame was meant (or could not stage);
        returns max_side"""
        from ._lib import RESIZE_MAX_LDS_BYTES, resize_lds_bytes
        hw, offset = torch.as_tensor(hw), torch.as_tensor(offset)
        if hw.dim() != 2 or hw.shape[1] != 2 or offset.dim() != 1 or offset.shape[0] != hw.shape[0] or hw.shape[0] == 0:
            raise ValueError(f"offset {tuple(offset.shape)} and hw {tuple(hw.shape)}: (F,) and (F, 2), F > 0")
        h, w = hw[:, 0].to(torch.int64), hw[:, 1].to(torch.int64)
        if int(h.min()) < 0 or int(w.min()) < 0:
            raise ValueError("a frame of negative size")
        there = (h > 0) & (w > 0)
        off, end = offset.to(torch.int64), offset.to(torch.int64) + h * w * self.channels
        if bool((there & ((off < 0) | (end > int(nbytes)))).any()):
            raise ValueError(f"a frame's bytes lie outside the buffer of {int(nbytes)} bytes")
        max_side = max(1, int(torch.where(there, torch.maximum(h, w), torch.zeros_like(h)).max()))
        if resize_lds_bytes(max_side, self.channels, self.size) > RESIZE_MAX_LDS_BYTES:
            raise ValueError(f"frames of up to {max_side} pixels a side and {self.channels} channels to size {self.size} need more "
                             "LDS than sfk_u8_pad_resize_cubic stages (include/sfk_resize.h)")
        return max_side

    def __call__(self, raw_bytes: torch.Tensor, offset: torch.Tensor, hw: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert raw_bytes.dtype == torch.uint8 and raw_bytes.dim() == 1
        offset = torch.as_tensor(offset).to(torch.int64).reshape(-1)
        hw = torch.as_tensor(hw).to(torch.int32).reshape(-1, 2)
        max_side = self.check_table(int(raw_bytes.numel()), offset, hw)
        f, s, c = int(hw.shape[0]), self.size, self.channels
        if out is None:
            out = torch.empty(f, s, s, c, dtype=torch.uint8, device=self.device)
        if raw_bytes.numel() == 0:              # every frame is missing: the kernel reads nothing, but wants a pointer
            raw_bytes = torch.zeros(1, dtype=torch.uint8)
            nbytes = 0
        else:
            nbytes = int(raw_bytes.numel())
        if raw_bytes.device.type == "cpu":
            self.bytes_uploaded += nbytes
        src = h2d(raw_bytes.contiguous(), self.device)
        stream = stream_of(self.device)
        self.be.u8_pad_resize_cubic(src[:nbytes] if nbytes else src, h2d(offset.contiguous(), self.device),
                                    h2d(hw.contiguous(), self.device), out, s, max_side, self.fill)(stream)
        return out


@dataclass(eq=False)
class U8Clip:
    """One pathway's view of a device uint8 batch, read by the stem kernels themselves (include/sfk_u8stem.h, MODEL.U8_STEM):
    the normalised, cropped float clip DevicePreprocess would write is never materialised.  Logical element (n, ci, t, h, w)
    is ``lut[frames[n, t, h + top - pad, w + left - pad, c0 + ci]]`` (zero outside the frame; no shift without a crop), the
    clip DevicePreprocess produces, sliced to channels c0 .. c0 + c - 1 and permuted to (N, c, T, H, W).

    frames: (N, T, H, W, P) uint8 with channel stride 1 and any pixel pitch P >= c0 + c (a loader may send only the
    channels the stems read); crop: (N, 2) int32 (top, left) on the same device, or None (test / valid clips).  The crop
    CONTENTS are read when the stems run, so a captured graph follows new offsets written into the same tensor."""
    frames: torch.Tensor
    c0: int
    c: int
    crop: Optional[torch.Tensor]
    pad: int
    lut: torch.Tensor

    def __post_init__(self):
        f = self.frames
        assert f.dtype == torch.uint8 and f.dim() == 5 and f.stride(4) == 1, "frames: (N, T, H, W, P) uint8, channels contiguous"
        assert 0 <= self.c0 and 0 < self.c and self.c0 + self.c <= f.shape[4] <= f.stride(3), (self.c0, self.c, f.shape)
        assert self.lut.dtype == torch.float32 and self.lut.numel() == 256 and self.lut.device == f.device
        if self.crop is not None:
            assert self.crop.dtype == torch.int32 and tuple(self.crop.shape) == (f.shape[0], 2) and self.crop.is_contiguous()
            assert self.crop.device == f.device

    # the logical (N, c, T, H, W) geometry, as the engine's plan code reads a float clip's
    @property
    def shape(self) -> torch.Size:
        n, t, h, w, _ = self.frames.shape
        return torch.Size((n, self.c, t, h, w))

    @property
    def device(self) -> torch.device:
        return self.frames.device

    @property
    def dtype(self) -> torch.dtype:
        return torch.uint8

    def dim(self) -> int:
        return 5

    def numel(self) -> int:
        return self.shape.numel()

    def element_size(self) -> int:
        return 1

    def geometry_key(self) -> tuple:
        """what a plan built for this clip depends on (never equal to a float tensor's key)"""
        f = self.frames
        return ("u8", tuple(f.shape), tuple(f.stride()), self.c0, self.c, self.crop is not None, self.pad)

    def bound_ptrs(self) -> tuple:
        """the device addresses the stem ops hold"""
        return (self.frames.data_ptr(), None if self.crop is None else self.crop.data_ptr(), self.lut.data_ptr())


@dataclass(eq=False)
class PoolClip:
    """``U8Clip``'s sibling for frames that lie in a ``FramePool``: one pathway's view of (arena, index table, crop table), read
    by the stem kernels themselves (include/sfk_u8stem_pool.h, MODEL.POOL_STEM), so the float clip ``FramePool.gather`` would
    write is never materialised.  Logical element (n, ci, t, h, w) is ``lut[arena[index[n, t], h + top - pad, w + left - pad,
    c0 + ci]]`` -- zero outside the frame, no shift without a crop, ``lut[fill]`` in place of the arena byte when index[n, t]
    is outside [0, F): the clip ``gather`` produces, sliced to channels c0 .. c0 + c - 1 and permuted to (N, c, T, H, W).

    arena: (F, H, W, P) uint8 with channel stride 1; index: (N, T) int32 and crop: (N, 2) int32 (top, left) or None, both on
    the arena's device.  Their CONTENTS are read when the stems run, so a captured graph follows new tables written into the
    same tensors, and a fixed-capacity arena hands every batch of an epoch the same addresses."""
    arena: torch.Tensor
    index: torch.Tensor
    c0: int
    c: int
    crop: Optional[torch.Tensor]
    pad: int
    lut: torch.Tensor
    fill: int

    def __post_init__(self):
        a, idx = self.arena, self.index
        assert a.dtype == torch.uint8 and a.dim() == 4 and a.stride(3) == 1, "arena: (F, H, W, P) uint8, channels contiguous"
        assert 0 <= self.c0 and 0 < self.c and self.c0 + self.c <= a.shape[3] <= a.stride(2), (self.c0, self.c, a.shape)
        assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.is_contiguous() and idx.device == a.device
        assert self.lut.dtype == torch.float32 and self.lut.numel() == 256 and self.lut.device == a.device
        assert 0 <= int(self.fill) <= 255 and self.pad >= 0
        if self.crop is not None:
            assert self.crop.dtype == torch.int32 and tuple(self.crop.shape) == (idx.shape[0], 2) and self.crop.is_contiguous()
            assert self.crop.device == a.device

    # the logical (N, c, T, H, W) geometry, as the engine's plan code reads a float clip's
    @property
    def shape(self) -> torch.Size:
        (n, t), (_, h, w, _) = self.index.shape, self.arena.shape
        return torch.Size((n, self.c, t, h, w))

    @property
    def device(self) -> torch.device:
        return self.arena.device

    @property
    def dtype(self) -> torch.dtype:
        return torch.uint8

    def dim(self) -> int:
        return 5

    def numel(self) -> int:
        return self.shape.numel()

    def element_size(self) -> int:
        return 1

    def geometry_key(self) -> tuple:
        """what a plan built for this clip depends on (never equal to a float tensor's or a U8Clip's key)"""
        a = self.arena
        return ("u8pool", tuple(a.shape), tuple(a.stride()), tuple(self.index.shape), self.c0, self.c, self.crop is not None,
                self.pad, self.fill)

    def bound_ptrs(self) -> tuple:
        """the device addresses the stem ops hold"""
        return (self.arena.data_ptr(), self.index.data_ptr(), None if self.crop is None else self.crop.data_ptr(),
                self.lut.data_ptr())


STEM_CLIPS = (U8Clip, PoolClip)                 # what a stem reads in place of a float tensor


def is_pool_clips(x) -> bool:
    """a batch entry that ``FramePool.clip`` made: a list of PoolClips, one per pathway"""
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(c, PoolClip) for c in x)


def u8_pathways(frames: torch.Tensor, crop: Optional[torch.Tensor], lut: torch.Tensor, channels) -> list:
    """U8Clips over the same device frames and crop, one per (c0, c) range; pad = S // 10 (RandomCrop's padding)."""
    pad = frames.shape[2] // 10
    return [U8Clip(frames, c0, c, crop, pad, lut) for c0, c in channels]


def byte_lut() -> torch.Tensor:
    """float32[256]: u / 255, the v2 loader's ``X.to(float32).div(255)`` (new_feature_test.py:600), bit for bit"""
    return torch.arange(256).float().div(255)


class RoiResize:
    """The v2 part-box loader's crop + /255 + Resize((S, S)) (new_feature_test.py:590-661) on the device: uint8 frames
    (N, T, H, W, C) and their boxes (N, 4) = (x1, y1, x2, y2) -> the (N, T, C, S, S) clip, f32 or bf16, in ONE
    ``sfk_roi_resize`` launch (include/sfk_v2.h).  The resize is ``F.interpolate(bilinear, align_corners=False,
    antialias=antialias)``, what torchvision's tensor ``Resize`` calls: pinned to torch, torchvision itself unpinned (it
    is not installed here; it antialiases tensors by default from 0.17 on and did not before).  crop (N, 2) int32
    (top, left) applies RandomCrop(S, padding) after the resize (``do_augment``), zeros outside.  warp (N, 6) float32
    (``draw_affine`` on S x S) instead of crop: every clip is the resize's own interpolant sampled through its matrix, by ONE
    ``sfk_roi_resize_warp`` launch (include/sfk_roi_warp.h) in place of the ``sfk_roi_resize`` one; the rows are validated on
    the host first (``validate_warp_rows``).  crop and warp together is a ValueError."""

    def __init__(self, size: int, device="cuda", backend=None, out_dtype: torch.dtype = torch.float32,
                 antialias: bool = True):
        self.be, self.device, self.out_dtype = hip_backend(backend), torch.device(device), out_dtype
        self.size, self.antialias = int(size), bool(antialias)
        self.lut = byte_lut().to(self.device)

    def __call__(self, frames_u8: torch.Tensor, box: torch.Tensor, crop: Optional[torch.Tensor] = None,
                 padding: Optional[int] = None, out: Optional[torch.Tensor] = None,
                 warp: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 5
        n, t, h, w, c = frames_u8.shape
        box, crop, pad, warp = _roi_tables("RoiResize", n, self.size, box, crop, padding, warp)
        x, box = h2d(frames_u8, self.device), h2d(box, self.device)
        if out is None:
            out = torch.empty(n, t, c, self.size, self.size, dtype=self.out_dtype, device=self.device)
        stream = stream_of(self.device)
        if warp is not None:
            self.be.roi_resize_warp(x, self.lut, box, h2d(warp, self.device), out, self.antialias)(stream)
            return out
        self.be.roi_resize(x, self.lut, box, out, self.antialias, None if crop is None else h2d(crop, self.device), pad)(stream)
        return out


# ---- the device-resident train set (MODEL.RESIDENT_TRAIN)
RESIDENT_METHODS = ("seq_len", "label", "video_item")


def offers_resident(train_set, methods=RESIDENT_METHODS) -> bool:
    """does the dataset offer the cheap methods a resident set reads it through (default: ``ResidentTrainSet``'s three)?"""
    return all(callable(getattr(train_set, m, None)) for m in methods)


class _VideoRequests(torch.utils.data.Dataset):
    """the reads an epoch of a resident set still needs, in plan order: (video, None, rect) = the whole video, (video,
    indices, rect) = those frames only; rect = (x1, y1, x2, y2) keeps only that rectangle of the frames under crop_key (a
    slice made here, in the loader worker), None keeps them whole.  A DataLoader over it lets workers decode ahead of the
    step that consumes them"""

    def __init__(self, train_set, requests, crop_key: Optional[str] = None):
        self.train_set, self.requests, self.crop_key = train_set, requests, crop_key

    def __len__(self):
        return len(self.requests)

    def __getitem__(self, k):
        i, indices, rect = self.requests[k]
        item = self.train_set.video_item(i) if indices is None else self.train_set.video_item(i, indices)
        if rect is not None:
            x1, y1, x2, y2 = rect
            item = dict(item)
            item[self.crop_key] = item[self.crop_key][:, y1:y2, x1:x2].contiguous()
        return item


class _ResidentSet:
    """What ``ResidentTrainSet`` (v1) and ``ResidentGestureSet`` (v2) share: one ``FramePool(capacity=)`` arena, a
    deterministic sampling plan drawn here, in the main process, the residency and spill rules and the epoch loop.  A derived
    class says what a clip's plan rows are beside its frame indices (``_clip_rows``), how a dataset item enters the pool
    (``_upload``) and how a batch is gathered from the arena slots (``_batch``).

    Plan: a function of (seed, epoch) only.  ``plan(e)`` = the batches of torch.randperm(len, manual_seed(seed + e)), each
    (videos, indices (N, T), <the derived class's columns>, jitter (N, 8) | None); per clip a generator seeded from (seed,
    epoch, video) draws the start (random_sampling: randint(0, max(0, seq_len - clip_len)), indices (start + k) % seq_len),
    then the derived class's draws, then, under MODEL.COLOR_JITTER, the jitter row (``draw_color_jitter``).
    Residency: decided in plan order and never revoked.  A video met for the first time becomes resident if resident_used +
    seq_len(i) still fits the resident region: it is read whole, once, and kept for the life of this object.  One that does
    not fit is spilled: only its clip's distinct frames are read, into slots released right after the batch's gather is
    enqueued (stream order keeps them intact until that gather has run).  Within a batch the resident uploads precede the
    spilled ones, so the resident videos pack densely from slot 0 and the spills never fragment their region.
    Counters: bytes_uploaded (the pool's), resident_videos, resident_frames (arena slots they hold), spilled_clips (of the
    epoch running or last run), spill_peak (most spill slots ever live at once).
    The residency rule is written over a per-video COST in the arena's own unit (``_cost``: seq_len slots here; a derived
    class whose arena is measured in bytes says so), a request may name the rectangle of the frames it needs (``_request``)
    and the table a batch is gathered from holds whatever ``_add`` returns per frame (slots here)."""
    methods = RESIDENT_METHODS                  # what the train set must offer
    lazy_batch = False                          # the batch reads the arena when the STEP runs (MODEL.POOL_STEM), not in _batch
    table_dtype = torch.int32                   # of the per-frame arena rows _add returns
    crop_key = None                             # the item entry a request's rectangle crops

    def __init__(self, train_set, cfg, device, backend, batch_size, drop_last, seed, num_workers, jitter):
        if not offers_resident(train_set, self.methods):
            raise ValueError(f"{type(self).__name__}: the train set must offer " + ", ".join(
                f"{m}(i, indices=None)" if m == "video_item" else f"{m}(i)" for m in self.methods))
        self.train_set, self.cfg, self.device, self.backend = train_set, cfg, torch.device(device), backend
        self.clip_len = int(cfg.CHALEARN.CLIP_LEN)
        self.batch_size, self.drop_last, self.seed = int(batch_size), bool(drop_last), int(seed)
        self.num_workers, self.jitter = int(num_workers), (None if jitter is None else tuple(jitter))
        self._seq_len = {}                      # video -> seq_len(i), asked once
        self._resident = {}                     # video -> True (resident) | False (spilled for good), in decision order
        self._rows = {}                         # loaded resident video -> (seq_len,) int32 arena slot of every frame, -1 missing
        self.resident_used = 0                  # sum of _cost over the videos decided resident
        self.resident_frames = 0
        self.spilled_clips = 0
        self.spill_peak = 0

    def _make_pool(self, capacity_frames: int) -> None:
        """the arena of capacity_frames slots: the last batch_size * CLIP_LEN of them are the spill region"""
        self.capacity, self.spill_slots = int(capacity_frames), self.batch_size * self.clip_len
        self.resident_slots = self.capacity - self.spill_slots
        if self.resident_slots <= 0:
            raise ValueError(f"{type(self).__name__}: {self.capacity} arena frames leave no resident slot beside the spill region "
                             f"of batch_size * CLIP_LEN = {self.spill_slots}")
        self.pool = FramePool(self.device, self.backend, capacity=self.capacity)

    # ---- counters
    @property
    def bytes_uploaded(self) -> int:
        return self.pool.bytes_uploaded

    @property
    def resident_videos(self) -> int:
        return len(self._rows)

    # ---- the plan: pure host
    def seq_len(self, i: int) -> int:
        if i not in self._seq_len:
            self._seq_len[i] = int(self.train_set.seq_len(i))
            assert self._seq_len[i] >= 1, (i, self._seq_len[i])
        return self._seq_len[i]

    def _clip_generator(self, epoch: int, video: int) -> torch.Generator:
        return torch.Generator().manual_seed(((self.seed * 1000003 + int(epoch)) * 1000003 + int(video)) % (2 ** 63 - 1))

    def plan(self, epoch: int) -> list:
        n = len(self.train_set)
        order = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + int(epoch))).tolist()
        batches = []
        for at in range(0, n, self.batch_size):
            videos = order[at:at + self.batch_size]
            if len(videos) < self.batch_size and self.drop_last:
                break
            indices, rows, jitter = [], [], []
            for v in videos:
                g, length = self._clip_generator(epoch, v), self.seq_len(v)
                start = int(torch.randint(0, max(0, length - self.clip_len) + 1, (1,), generator=g))
                indices.append([(start + k) % length for k in range(self.clip_len)])
                rows.append(self._clip_rows(g, v, indices[-1]))
                if self.jitter is not None:
                    jitter.append(draw_color_jitter(1, *self.jitter, generator=g)[0])
            columns = tuple(None if col[0] is None else torch.stack(col) for col in zip(*rows))
            batches.append((videos, torch.tensor(indices, dtype=torch.int32)) + columns
                           + (torch.stack(jitter) if jitter else None,))
        return batches

    # ---- residency and loading
    def _cost(self, video: int) -> Optional[int]:
        """what the video would hold of the resident region, in the arena's unit; None: it can only be spilled"""
        return self.seq_len(video)

    def _request(self, entry, n: int, indices) -> tuple:
        """the read of clip n of a plan entry: its whole video (indices None) or those frames only"""
        return (entry[0][n], indices, None)

    def _live_frames(self, base: int) -> int:
        return self.pool.live[base]

    def _decide(self, video: int) -> bool:
        if video not in self._resident:
            cost = self._cost(video)
            fits = cost is not None and self.resident_used + cost <= self.resident_slots
            self._resident[video] = fits
            if fits:
                self.resident_used += cost
        return self._resident[video]

    def _drain(self) -> None:
        """wait for everything enqueued on the device (every stream: the stems may run on the engine's side streams)"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _add(self, item) -> tuple:
        """(base, (L,) int32 arena slot of every requested frame, -1 for a missing one) of a dataset item"""
        windows = torch.as_tensor(item["windows"], dtype=torch.int32)
        base = self._upload(item, windows)
        return base, self.pool.rows(base, windows)[0]

    def epoch(self, epoch: int):
        plan = self.plan(epoch)
        requests, per_batch = [], []            # per batch: (videos that become resident now, [(clip n, distinct indices)])
        for entry in plan:
            videos, indices = entry[0], entry[1]
            new, spill = [], []
            for n, v in enumerate(videos):
                if self._decide(v):
                    if v not in self._rows:     # (a video occurs once an epoch: the order is a permutation)
                        new.append(n)
                else:
                    spill.append((n, sorted(set(indices[n].tolist()))))
            requests += [self._request(entry, n, None) for n in new] + [self._request(entry, n, ind) for n, ind in spill]
            per_batch.append(([videos[n] for n in new], spill))
        items = None
        if requests:                            # an epoch with nothing to read builds no loader
            items = iter(torch.utils.data.DataLoader(_VideoRequests(self.train_set, requests, self.crop_key), batch_size=None,
                                                     shuffle=False, num_workers=self.num_workers))
        self.spilled_clips = 0
        for entry, (new, spill) in zip(plan, per_batch):
            videos, indices, jitter = entry[0], entry[1], entry[-1]
            for v in new:                       # the resident uploads first: no spill slot is live, they pack densely
                base, rows = self._add(next(items))
                assert rows.numel() == self.seq_len(v), (v, rows.numel(), self.seq_len(v))
                self._rows[v] = rows
                self.resident_frames += self._live_frames(base)
            table, bases = torch.empty(indices.shape, dtype=self.table_dtype), []
            spilled = dict(spill)
            for n, v in enumerate(videos):
                if n in spilled:
                    base, rows = self._add(next(items))
                    bases.append(base)
                    slot = dict(zip(spilled[n], rows.tolist()))
                    table[n] = torch.tensor([slot[k] for k in indices[n].tolist()], dtype=self.table_dtype)
                else:
                    table[n] = self._rows[v][indices[n].long()]
            self.spilled_clips += len(bases)
            self.spill_peak = max(self.spill_peak, sum(self._live_frames(b) for b in bases))
            batch = self._batch(table, entry)
            if not self.lazy_batch:
                for b in bases:                 # free for the uploads queued behind that gather on the same stream
                    self.pool.release(b)
            batch["label"] = torch.tensor([int(self.train_set.label(v)) for v in videos], dtype=torch.int64)
            if jitter is not None:
                batch["jitter"] = jitter
            if not self.lazy_batch:
                yield batch
                continue
            # the batch reads the arena when its step runs, so the slots go back only when the consumer leaves this yield.  It
            # comes back for the next batch: the step that reads these slots (and the tables) has been enqueued, the next
            # uploads queue behind it.  It stops here instead -- a break, an exception, the generator dropped: the release
            # still happens (the bookkeeping is that of the gathered route), but what was enqueued is not known to be on the
            # stream later uploads take, so the device is drained first.  A batch not yet stepped is void from then on.
            resumed = False
            try:
                yield batch
                resumed = True
            finally:
                if not resumed:
                    self._drain()
                for b in bases:
                    self.pool.release(b)


class ResidentTrainSet(_ResidentSet):
    """The train set of the v1 loader with its decoded frames kept on the device (the machinery: ``_ResidentSet``).  The
    reference's train loop draws one random window per video per epoch (dataset/chalearn_dataset.py:123-129) and decodes its
    frames again every time; here a video is decoded ONCE, when a clip first touches it, and every batch after that is one
    ``sfk_u8_pool_gather_crop`` launch (include/sfk_resident.h) plus the H2D of two small tables.

    train_set offers ``seq_len(i)`` (frame names of video i, nothing read), ``label(i)`` (0-based) and ``video_item(i,
    indices=None)`` (``make_pooled_item`` / ``make_raw_pooled_item`` over those frames, default all, 'windows' of shape
    (1, len(indices))).

    Arena: capacity_frames slots (default floor(MODEL.RESIDENT_GB * 2^30 / (S*S*21))); the last batch_size * CLIP_LEN of
    them are the spill region, the rest the resident region.
    Plan: ``plan(e)`` batches are (videos, indices (N, T), crop (N, 2), jitter (N, 8) | None); per clip the start, then the
    crop (``draw_crop_offsets``), then the jitter row.  affine = (degrees, (lo, hi), shear, flip) (MODEL.AFFINE): the third
    column is the (N, 6) float32 warp row of ``draw_affine`` instead, told from the int32 crop rows by its dtype, and a batch
    is one ``sfk_u8_pool_gather_warp`` launch (include/sfk_warp.h); with stem_channels it is a ValueError (no float clip).
    ``epoch(e)`` yields {'<key>': (N, T, 21, S, S) float32 on the device, 'label': (N,), optionally 'jitter': (N, 8)}: what
    every model's prepare_data takes under the float key (like pooled eval, whatever MODEL.U8_STEM says).
    stem_channels (MODEL.POOL_STEM): the (c0, c) channel range of every pathway's stem.  '<key>' is then the list of
    ``PoolClip``s ``FramePool.clip`` makes -- no launch, no float clip; the stems read the arena when the step runs, so a
    spilled clip's slots are released when the consumer comes back for the next batch, after it has enqueued that step."""

    def __init__(self, train_set, cfg, device="cuda", backend=None, batch_size: int = 1, drop_last: bool = True, seed: int = 0,
                 capacity_frames: Optional[int] = None, num_workers: int = 0, jitter=None, stem_channels=None, affine=None):
        super().__init__(train_set, cfg, device, backend, batch_size, drop_last, seed, num_workers, jitter)
        from .config import crop_resize_dict
        self.key = cfg.MODEL.R3D_INPUT
        # MODEL.AFFINE: (degrees, (scale lo, hi), shear, flip) -- the plan's third column is then the warp row, not the crop row
        self.affine = None if affine is None else (float(affine[0]), tuple(float(v) for v in affine[1]), float(affine[2]),
                                                   float(affine[3]))
        if self.affine is not None and stem_channels is not None:
            raise ValueError("ResidentTrainSet: MODEL.POOL_STEM reads the uint8 frames in the stems, so there is no float clip "
                             "for MODEL.AFFINE to sample; turn POOL_STEM or AFFINE off")
        # MODEL.POOL_STEM: the (c0, c) range each pathway's stem reads; the batch is then those PoolClips, not the float clip
        self.stem_channels = None if stem_channels is None else [(int(c0), int(c)) for c0, c in stem_channels]
        self.lazy_batch = self.stem_channels is not None
        self.size = int(crop_resize_dict[self.key])
        if capacity_frames is None:
            capacity_frames = int(float(cfg.MODEL.RESIDENT_GB) * 2 ** 30 // (self.size * self.size * 21))
        self._make_pool(capacity_frames)

    def _clip_rows(self, g, video, indices) -> tuple:
        if self.affine is not None:             # the same stream position for (top, left) as the crop row's
            return (draw_affine(1, self.size, self.size // 10, *self.affine, generator=g)[0],)
        return (draw_crop_offsets(1, self.size // 10, g)[0],)

    def _upload(self, item, windows) -> int:
        if rawpool_key(self.key) in item:
            return self.pool.add_raw(item[rawpool_key(self.key)], item["raw_hw"], self.size, windows)
        return self.pool.add(item[pool_key(self.key)], windows)

    def _batch(self, table, entry) -> dict:
        if self.stem_channels is not None:
            return {self.key: self.pool.clip(table, self.stem_channels, crop=entry[2])}
        if entry[2].dtype == torch.float32:     # (N, 6) warp rows (MODEL.AFFINE); the crop rows are (N, 2) int32
            return {self.key: self.pool.gather(table, torch.float32, 0, None, warp=entry[2])}
        return {self.key: self.pool.gather(table, torch.float32, 0, None, crop=entry[2])}


GESTURE_METHODS = RESIDENT_METHODS + ("frame_boxes",)
NO_BOX = (2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31)   # frame_boxes' row of a frame without any of the parts: min/max ignore it


class ResidentGestureSet(_ResidentSet):
    """The train set of the v2 part-box loader (gesture_v2.py) with its decoded, UNCROPPED frames kept on the device (the
    machinery: ``_ResidentSet``).  The reference decodes five videos per clip in every epoch (new_feature_test.py:590-606);
    here a video is decoded once and every batch after that is one ``sfk_roi_resize_pool`` launch (include/sfk_roi_pool.h)
    plus the H2D of its index, box and, when augmenting, crop tables.

    train_set offers ``seq_len(i)``, ``label(i)`` (0-based), ``video_item(i, indices=None)`` = {'frames_pool': (L, H, W, 7)
    uint8 [R, G, B, U, V, F0, F1] of those frames (default all), 'windows': (1, L)} and ``frame_boxes(i)`` = (seq_len, 4) int32,
    a frame's union box over MODEL.PARTS, ``NO_BOX`` for a frame with none of them; frame_boxes is asked once per video.

    Arena: frames of (H, W, 7), the shape of frame 0 of video 0, read once when this object is built; capacity_frames slots
    (default floor(MODEL.RESIDENT_GB * 2^30 / (H*W*7))), the last batch_size * CLIP_LEN of them the spill region.
    Plan: ``plan(e)`` batches are (videos, indices (N, T), box (N, 4), crop (N, 2) | None, jitter (N, 8) | None); per clip the
    start exactly as v1 draws it, the crop row (``draw_crop_offsets``, padding S // 10) only with augment=True (the reference
    trains with do_augment=False, new_feature_test.py:814), then the jitter row.  affine = (degrees, (lo, hi), shear, flip)
    (MODEL.AFFINE): the crop column holds the (6,) float32 warp row of ``draw_affine(1, S, S // 10, ...)`` instead, drawn at
    the crop row's stream position (its first two draws ARE the crop's), told from the int32 crop rows by its dtype; a batch
    is then one ``sfk_roi_resize_pool_warp`` / ``sfk_roi_resize_ragged_warp`` launch (include/sfk_roi_warp.h).  The matrix
    lives in the resized image's coordinates, so both stores give the same batches.  A clip's box is the min / max over the
    frame_boxes rows of its indices, clamped as ``ChalearnGestureFrames.clip_box`` clamps it; an empty one is a ValueError
    naming the video, raised by ``plan``.
    ``epoch(e)`` yields {'clip_v2': (N, T, 7, S, S) on the device in MODEL.DTYPE, 'label': (N,), optionally 'jitter': (N, 8)},
    S = MODEL.INPUT_SIZE, resized with MODEL.RESIZE_ANTIALIAS: what ``RoiResize`` writes from the same frames and boxes.

    store='box' (MODEL.RESIDENT_STORE) keeps of every video only what its clips can read: the rectangle R_v = the union of
    frame_boxes(v), clamped as ``clip_box`` clamps.  The arena is then a ``BoxArena`` of capacity_bytes (default
    floor(MODEL.RESIDENT_GB * 2^30); capacity_frames, when given instead, counts whole frames), its last batch_size *
    (CLIP_LEN * H*W*7 + 16) bytes the spill region; a video costs seq_len * h_R * w_R * 7 bytes rounded up to 16, decided in
    plan order as above; a spilled clip uploads its distinct frames cropped to the clip's OWN box.  The crop is a slice in
    the loader worker; a batch is one ``sfk_roi_resize_ragged`` launch (include/sfk_roi_ragged.h) with each clip's box
    translated by its rectangle's origin.  Same plan, same batches bit for bit: a resize reads nothing outside its box.  A
    video without any part box can only be spilled (and ``plan`` raises for its clips).  ``resident_bytes_used``: the arena
    bytes the resident videos hold, under either store."""
    methods = GESTURE_METHODS
    key = "frames"                              # video_item's pool entry is pool_key(key)

    def __init__(self, train_set, cfg, device="cuda", backend=None, batch_size: int = 1, drop_last: bool = False, seed: int = 0,
                 capacity_frames: Optional[int] = None, num_workers: int = 0, jitter=None, augment: bool = False,
                 store: Optional[str] = None, capacity_bytes: Optional[int] = None, affine=None):
        super().__init__(train_set, cfg, device, backend, batch_size, drop_last, seed, num_workers, jitter)
        # MODEL.AFFINE: (degrees, (scale lo, hi), shear, flip) -- the plan's crop column is then the warp row
        self.affine = None if affine is None else (float(affine[0]), tuple(float(v) for v in affine[1]), float(affine[2]),
                                                   float(affine[3]))
        self.store = str(cfg.MODEL.get("RESIDENT_STORE", "frame") if store is None else store)
        if self.store not in ("frame", "box"):
            raise ValueError(f"ResidentGestureSet: store {self.store!r} is neither 'frame' nor 'box'")
        if capacity_bytes is not None and self.store != "box":
            raise ValueError("ResidentGestureSet: capacity_bytes is the 'box' store's; the 'frame' store counts capacity_frames")
        from .slowfast import _DTYPES
        self.size, self.augment = int(cfg.MODEL.INPUT_SIZE), bool(augment)
        self.out_dtype = _DTYPES[str(cfg.MODEL.get("DTYPE", "fp32")).lower()]
        self.antialias = bool(cfg.MODEL.get("RESIZE_ANTIALIAS", True))
        probe = train_set.video_item(0, [0])[pool_key(self.key)]
        assert probe.dtype == torch.uint8 and probe.dim() == 4 and probe.shape[0] == 1, (probe.dtype, tuple(probe.shape))
        self.frame_shape = tuple(int(v) for v in probe.shape[1:])
        h, w, p = self.frame_shape
        self._boxes = {}                        # video -> frame_boxes(i), asked once
        if self.store == "box":
            if capacity_bytes is None:
                capacity_bytes = (int(float(cfg.MODEL.RESIDENT_GB) * 2 ** 30) if capacity_frames is None
                                  else int(capacity_frames) * h * w * p)
            self._make_arena(capacity_bytes)
            return
        if capacity_frames is None:
            capacity_frames = int(float(cfg.MODEL.RESIDENT_GB) * 2 ** 30 // (h * w * p))
        self._make_pool(capacity_frames)

    # ---- store='box': the arena in bytes, a video's rectangle, its cost, its requests
    def _make_arena(self, capacity_bytes: int) -> None:
        """the arena of capacity_bytes: its last batch_size * (CLIP_LEN * H*W*P + 16) bytes, the worst case of whole frames,
        are the spill region (``capacity``, ``spill_slots`` and ``resident_slots`` count bytes under this store)"""
        h, w, p = self.frame_shape
        self.capacity = int(capacity_bytes) // BoxArena.ALIGN * BoxArena.ALIGN
        self.spill_slots = self.batch_size * (self.clip_len * h * w * p + BoxArena.ALIGN)
        self.resident_slots = self.capacity - self.spill_slots
        if self.resident_slots <= 0:
            raise ValueError(f"ResidentGestureSet: {capacity_bytes} arena bytes leave no resident byte beside the spill region of "
                             f"batch_size * (CLIP_LEN * H*W*{p} + {BoxArena.ALIGN}) = {self.spill_slots}")
        self.pool = BoxArena(self.capacity, self.device, self.backend)
        self.table_dtype, self.crop_key = torch.int64, pool_key(self.key)
        self._rects = {}                        # video -> R_v (x1, y1, x2, y2) | None

    @property
    def resident_bytes_used(self) -> int:
        """the arena bytes the loaded resident videos hold"""
        h, w, p = self.frame_shape
        if self.store != "box":
            return self.resident_frames * h * w * p
        return sum(self.seq_len(v) * (r[3] - r[1]) * (r[2] - r[0]) * p for v in self._rows for r in [self.video_rect(v)])

    def video_rect(self, video: int) -> Optional[tuple]:
        """R_v = (x1, y1, x2, y2): the union of the video's frame boxes, clamped to the frame as ``clip_box`` clamps; None
        when it is empty (no frame has a part, or the union misses the frame)"""
        if video not in self._rects:
            b = self.frame_boxes(video)
            h, w = self.frame_shape[:2]
            x1, y1 = max(0, int(b[:, 0].min())), max(0, int(b[:, 1].min()))
            x2, y2 = min(int(b[:, 2].max()), w), min(int(b[:, 3].max()), h)
            self._rects[video] = None if x2 <= x1 or y2 <= y1 else (x1, y1, x2, y2)
        return self._rects[video]

    def _cost(self, video: int) -> Optional[int]:
        if self.store != "box":
            return super()._cost(video)
        r = self.video_rect(video)
        if r is None:
            return None
        nbytes = self.seq_len(video) * (r[3] - r[1]) * (r[2] - r[0]) * self.frame_shape[2]
        return -(-nbytes // BoxArena.ALIGN) * BoxArena.ALIGN

    def _request(self, entry, n: int, indices) -> tuple:
        if self.store != "box":
            return super()._request(entry, n, indices)
        return (entry[0][n], indices, self.video_rect(entry[0][n]) if indices is None else tuple(entry[2][n].tolist()))

    def _live_frames(self, base: int) -> int:
        return self.pool.live[base][0] if self.store == "box" else super()._live_frames(base)

    def _add(self, item) -> tuple:
        if self.store != "box":
            return super()._add(item)
        windows = torch.as_tensor(item["windows"], dtype=torch.int32)
        frames = item[pool_key(self.key)]
        FramePool.check_windows(windows, int(frames.shape[0]))
        base = self.pool.add(frames)
        return base, self.pool.offsets(base, windows)[0]

    def frame_boxes(self, i: int) -> torch.Tensor:
        if i not in self._boxes:
            b = torch.as_tensor(self.train_set.frame_boxes(i)).to(torch.int32)
            assert tuple(b.shape) == (self.seq_len(i), 4), (i, tuple(b.shape), self.seq_len(i))
            self._boxes[i] = b
        return self._boxes[i]

    def clip_box(self, video: int, indices) -> torch.Tensor:
        """int32 (x1, y1, x2, y2): the union of the clip's frame boxes, clamped to the frame"""
        b = self.frame_boxes(video)[torch.as_tensor(indices, dtype=torch.long)]
        h, w = self.frame_shape[:2]
        x1, y1, x2, y2 = int(b[:, 0].min()), int(b[:, 1].min()), int(b[:, 2].max()), int(b[:, 3].max())
        if x1 > x2:                             # every row is NO_BOX
            raise ValueError(f"video {video}: no part box in any frame of the clip {list(indices)}")
        x1, y1, x2, y2 = max(0, x1), max(0, y1), min(x2, w), min(y2, h)
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"video {video}: empty part box {(x1, y1, x2, y2)} in a {w}x{h} frame")
        return torch.tensor([x1, y1, x2, y2], dtype=torch.int32)

    def _clip_rows(self, g, video, indices) -> tuple:
        if self.affine is not None:             # the same stream position for (top, left) as the crop row's
            return (self.clip_box(video, indices), draw_affine(1, self.size, self.size // 10, *self.affine, generator=g)[0])
        return (self.clip_box(video, indices), draw_crop_offsets(1, self.size // 10, g)[0] if self.augment else None)

    def _upload(self, item, windows) -> int:
        return self.pool.add(item[pool_key(self.key)], windows)

    def _batch(self, table, entry) -> dict:
        # (N, 6) float32 warp rows (MODEL.AFFINE); the crop rows are (N, 2) int32
        aug = dict(warp=entry[3]) if entry[3] is not None and entry[3].dtype == torch.float32 else dict(crop=entry[3])
        if self.store == "box":
            # a resident video's frames lie in R_v, a spilled clip's in its own box: translate each box by that origin
            rect = torch.tensor([self.video_rect(v) if self._resident[v] else entry[2][n].tolist() for n, v in enumerate(entry[0])],
                                dtype=torch.int32)
            hw = torch.stack([rect[:, 3] - rect[:, 1], rect[:, 2] - rect[:, 0]], 1)
            box = entry[2] - torch.cat([rect[:, :2], rect[:, :2]], 1)
            return {"clip_v2": self.pool.roi_gather(table, hw, box, self.size, self.out_dtype, self.antialias, **aug)}
        return {"clip_v2": self.pool.roi_gather(table, entry[2], self.size, self.out_dtype, self.antialias, **aug)}
