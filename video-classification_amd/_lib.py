"""ctypes binding of include/sfk.h and the HIP backend the engine drives.

There is NO fallback: if libsfk.so is missing or fails to load, ``load()`` raises.  The engine talks to a
*backend* object whose methods mirror the C entry points and return zero-allocation closures ``run(stream)``
with every descriptor pre-built, so a training step is a flat list of C calls on one hipStream (and can be
captured into a hipGraph).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFK_LIB") or os.path.join(HERE, "libsfk.so")   # SFK_LIB: experiment builds (tools/gpu_ab_lib.sh)
SFK_F32, SFK_BF16 = 0, 1
SFK_MAX_TAPS = 16
ABI_VERSION = 24       # include/sfk.h SFK_ABI_VERSION
BN_FOLD_ROWS = 64      # include/sfk.h SFK_BN_FOLD_ROWS
_DT = {torch.float32: SFK_F32, torch.bfloat16: SFK_BF16}


class SfkError(RuntimeError):
    pass


# ----------------------------------------------------------------------------- python-side descriptors
@dataclass
class FMap:
    """Channels-last feature map view: element (n,t,h,w,c) at buf[(((n*T+t)*H+h)*W+w)*ld + c_off + c]."""
    buf: torch.Tensor
    n: int
    t: int
    h: int
    w: int
    c: int
    ld: int = 0
    c_off: int = 0

    def __post_init__(self):
        if self.ld == 0:
            self.ld = self.c
        assert self.ld >= self.c_off + self.c
        assert self.buf.numel() >= self.pixels * self.ld, (self.buf.numel(), self.pixels, self.ld)

    @property
    def pixels(self) -> int:
        return self.n * self.t * self.h * self.w

    @property
    def dtype(self) -> torch.dtype:
        return self.buf.dtype

    def channels(self, c0: int, c: int) -> "FMap":
        assert 0 <= c0 and c0 + c <= self.c
        return FMap(self.buf, self.n, self.t, self.h, self.w, c, self.ld, self.c_off + c0)

    def view5(self) -> torch.Tensor:
        """(N,T,H,W,C) strided torch view of this map (for tests and host-side glue)."""
        return self.buf[: self.pixels * self.ld].view(self.n, self.t, self.h, self.w, self.ld)[
            ..., self.c_off:self.c_off + self.c]

    def like(self, buf: torch.Tensor, c: Optional[int] = None) -> "FMap":
        c = self.c if c is None else c
        return FMap(buf, self.n, self.t, self.h, self.w, c)


Tap = Tuple[int, int, int, int]  # (dt, dh, dw, widx)


@dataclass
class BnBwdFuse:
    """sfk_bn_bwd_fuse: the BatchNorm-backward reduce folded into the data-gradient pass that produces dA."""
    y_bn: Optional[FMap]             # conv output the BatchNorm normalised; None (+ relu_out_bits): bitmap mask, sum dz only
    mask_src: Optional[FMap]         # activation whose sign is the ReLU mask, or None
    mean: Optional[torch.Tensor]
    invstd: Optional[torch.Tensor]
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    relu: bool
    partials: torch.Tensor           # fp32 [mtiles][cout][2]


@dataclass
class ConvEpilogue:
    """sfk_conv_epilogue: v = acc*scale + shift (+ old y) (+ res*res_scale + res_shift); ReLU (+ bitmap); y = v."""
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    res: Optional[FMap] = None
    res_scale: Optional[torch.Tensor] = None
    res_shift: Optional[torch.Tensor] = None
    relu: bool = False
    relu_bits: Optional[torch.Tensor] = None


@dataclass
class ConvPass:
    x: FMap
    y: FMap
    rows: Tuple[int, int, int]
    gs: Tuple[int, int, int]
    os: Tuple[int, int, int]
    oo: Tuple[int, int, int]
    taps: List[Tap]
    w: torch.Tensor          # [cout][wtaps][cin] flat, dtype of x
    wtaps: int
    cin: int
    cout: int
    accumulate: bool = False
    stats: Optional[torch.Tensor] = None  # fp32 [mtiles][cout][2]
    bnb: Optional[BnBwdFuse] = None
    relu_out_bits: Optional[torch.Tensor] = None   # uint8 bitmap of bn_apply: the pass stores result * mask
    ep: Optional[ConvEpilogue] = None


@dataclass
class WgradPass:
    x: FMap
    dy: FMap
    gs: Tuple[int, int, int]
    taps: List[Tap]
    dw: torch.Tensor         # fp32 [cout][wtaps][cin] flat view into the gradient arena
    wtaps: int
    cin: int
    cout: int
    workspace: Optional[torch.Tensor] = None   # fp32 scratch for the partial-tile path (sfk_conv_wgrad_workspace_bytes)
    dg_w: Optional[torch.Tensor] = None        # fused data gradient of the same dY: [cin][cout] matrix (include/sfk.h)
    dg_y: Optional[FMap] = None                # ... its output map (cin channels)


@dataclass
class StemSrc:
    src: torch.Tensor        # any strided view indexed (n, c, t, h, w), f32 or bf16, read in place (or an input_pipeline
                             # U8Clip / PoolClip: the u8stem* / u8pstem* entry points)
    t_index: Optional[torch.Tensor]   # int32 frame indices (PackPathway) or None
    kt: int

    @property
    def t_len(self) -> int:
        return int(self.t_index.numel()) if self.t_index is not None else int(self.src.shape[2])


def stem_kp(cin: int, kt: int) -> int:
    """row length of the stem filter layout [co][((f*cin+ci)*7+kh)*8+kw] (mirrors sfk_stem_kp)"""
    return (kt * cin * 7 + 3) // 4 * 4 * 8


# ----------------------------------------------------------------------------- ctypes mirror of sfk.h
class _FMap(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("c", C.c_int32), ("ld", C.c_int32), ("c_off", C.c_int32)]


class _Tap(C.Structure):
    _fields_ = [("dt", C.c_int8), ("dh", C.c_int8), ("dw", C.c_int8), ("widx", C.c_uint8)]


class _BnBwdFuse(C.Structure):
    _fields_ = [("y_bn", _FMap), ("mask_src", _FMap), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("relu", C.c_int32), ("partials", C.c_void_p)]


class _ConvEpilogue(C.Structure):
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("res", _FMap), ("res_scale", C.c_void_p),
                ("res_shift", C.c_void_p), ("relu", C.c_int32), ("reserved", C.c_int32), ("relu_bits", C.c_void_p)]


class _ConvDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("x", _FMap), ("y", _FMap), ("rt", C.c_int32), ("rh", C.c_int32), ("rw", C.c_int32),
                ("gs", C.c_int32 * 3), ("os", C.c_int32 * 3), ("oo", C.c_int32 * 3), ("ntaps", C.c_int32),
                ("taps", _Tap * SFK_MAX_TAPS), ("w", C.c_void_p), ("wtaps", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("accumulate", C.c_int32), ("stats", C.c_void_p), ("bnb", _BnBwdFuse),
                ("out_relu_bits", C.c_void_p), ("ep", _ConvEpilogue)]


class _WgradDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("x", _FMap), ("dy", _FMap), ("gs", C.c_int32 * 3), ("ntaps", C.c_int32),
                ("taps", _Tap * SFK_MAX_TAPS), ("dw", C.c_void_p), ("wtaps", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("dg_w", C.c_void_p), ("dg_y", _FMap)]


class _StemSrc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_dtype", C.c_int32), ("sn", C.c_int64), ("sc", C.c_int64),
                ("st", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("cin", C.c_int32), ("t_in", C.c_int32),
                ("h_in", C.c_int32), ("w_in", C.c_int32), ("t_index", C.c_void_p), ("t_len", C.c_int32),
                ("kt", C.c_int32)]


class _Stem2dSrc(C.Structure):
    """include/sfk_stem2d.h sfk_stem2d_src: element (n, t, c, h, w) at src[n*sn + t*st + c*sc + h*sh + w*sw]"""
    _fields_ = [("struct_size", C.c_uint32), ("src_dtype", C.c_int32), ("src", C.c_void_p), ("sn", C.c_int64),
                ("st", C.c_int64), ("sc", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("n", C.c_int32),
                ("t", C.c_int32), ("c", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32), ("reserved0", C.c_int32)]


class _U8Clip(C.Structure):
    """include/sfk_u8stem.h sfk_u8_clip: byte (n, t, y, x, ch) at src[n*sn + t*st + y*sh + x*sw + ch]; the stem reads
    channels c0 .. c0 + c - 1 through lut, shifted by the per-clip crop (or not)"""
    _fields_ = [("struct_size", C.c_uint32), ("pad", C.c_int32), ("src", C.c_void_p), ("sn", C.c_int64), ("st", C.c_int64),
                ("sh", C.c_int64), ("sw", C.c_int64), ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32),
                ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("lut", C.c_void_p), ("crop", C.c_void_p)]


class _U8PoolClip(C.Structure):
    """include/sfk_u8stem_pool.h sfk_u8_pool_clip: sfk_u8_clip with its frames in a frame pool -- byte (f, y, x, ch) at
    pool[f*frame_stride + y*row_stride + x*pixel_pitch + ch], frame t of clip n is pool frame index[n][t] (outside [0, frames):
    the constant image of byte fill); the stem reads channels c0 .. c0 + c - 1 through lut, shifted by the per-clip crop"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("c0", C.c_int32), ("c", C.c_int32),
                ("n", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("crop", C.c_void_p), ("pad", C.c_int32), ("fill", C.c_int32)]


class _RoiDesc(C.Structure):
    """include/sfk_v2.h sfk_roi_desc: byte (n, t, y, x, c) at src[n*sn + t*st + y*sh + x*sw + c*sc]; the resized crop of
    box[n] lands at dst[n*dn + t*dt + (c_off + c)*dc + y*dh + x]"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("src", C.c_void_p), ("sn", C.c_int64),
                ("st", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("sc", C.c_int64), ("n", C.c_int32),
                ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("lut", C.c_void_p), ("box", C.c_void_p), ("crop", C.c_void_p), ("pad", C.c_int32),
                ("dst_dtype", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64), ("dt", C.c_int64), ("dc", C.c_int64),
                ("dh", C.c_int64), ("c_off", C.c_int32), ("reserved0", C.c_int32)]


class _JitterDesc(C.Structure):
    """include/sfk_aug.h sfk_jitter_desc: element (n, t, c, y, x) of the three colour planes at
    x[n*sn + t*st + (c_off + c)*sc + y*sh + x], jittered in place with the per-clip params[n][8]"""
    _fields_ = [("struct_size", C.c_uint32), ("dtype", C.c_int32), ("x", C.c_void_p), ("sn", C.c_int64), ("st", C.c_int64),
                ("sc", C.c_int64), ("sh", C.c_int64), ("n", C.c_int32), ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c_off", C.c_int32), ("bgr", C.c_int32), ("mean", C.c_float), ("std", C.c_float), ("params", C.c_void_p),
                ("workspace", C.c_void_p)]


class _MixDesc(C.Structure):
    """include/sfk_mix.h sfk_mix_desc: element (n, t, c, y, x) of the c mixed channels at
    x[n*sn + t*st + (c_off + c)*sc + y*sh + x], mixed in place with its partner clip by the per-clip rows[n][8]"""
    _fields_ = [("struct_size", C.c_uint32), ("dtype", C.c_int32), ("x", C.c_void_p), ("sn", C.c_int64), ("st", C.c_int64),
                ("sc", C.c_int64), ("sh", C.c_int64), ("n", C.c_int32), ("t", C.c_int32), ("c", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("c_off", C.c_int32), ("rows", C.c_void_p)]


class _EmaTensor(C.Structure):
    """include/sfk_ema.h sfk_ema_tensor: a live tensor outside the arena and its average, n elements each"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32)]


class _EmaDesc(C.Structure):
    """include/sfk_ema.h sfk_ema_desc: the live arena p, its average e, the device table of small tensors, the rate and the
    device step counter shared by sfk_ema_update and sfk_ema_swap"""
    _fields_ = [("struct_size", C.c_uint32), ("warmup", C.c_int32), ("p", C.c_void_p), ("e", C.c_void_p), ("count", C.c_int64),
                ("table", C.c_void_p), ("ntensors", C.c_int32), ("reserved0", C.c_int32), ("decay", C.c_double),
                ("step", C.c_void_p)]


class _OptimHp(C.Structure):
    """include/sfk_optim.h sfk_optim_hp: the device learning-rate table, weight decay and clipping coefficient shared by
    sfk_adam_hp and sfk_sgd_hp"""
    _fields_ = [("struct_size", C.c_uint32), ("decay_mode", C.c_int32), ("lr_table", C.c_void_p), ("lr_len", C.c_int64),
                ("decay_count", C.c_int64), ("clip_coef", C.c_void_p), ("weight_decay", C.c_float), ("reserved0", C.c_int32)]


class _GroupSeg(C.Structure):
    """include/sfk_groups.h sfk_group_seg: arena elements [begin, end) of one parameter group"""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("tile0", C.c_int64), ("group", C.c_int32), ("decay", C.c_int32)]


class _GroupsHp(C.Structure):
    """include/sfk_groups.h sfk_groups_hp: the segment table (device copy and host mirror), the per-group rate rows and
    weight decays, the launch's decay mode and clipping coefficient"""
    _fields_ = [("struct_size", C.c_uint32), ("decay_mode", C.c_int32), ("segs", C.c_void_p), ("segs_host", C.c_void_p),
                ("nsegs", C.c_int32), ("ngroups", C.c_int32), ("lr_rows", C.c_void_p), ("lr_len", C.c_int64),
                ("weight_decay", C.c_void_p), ("clip_coef", C.c_void_p)]


class _PoolDesc(C.Structure):
    """include/sfk_pool.h sfk_pool_desc: byte (f, y, x, ch) of the frame pool at
    pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch]; clip n, time t of out is frame index[n][t] through lut"""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("fill", C.c_int32), ("out", C.c_void_p)]


class _PoolCropDesc(C.Structure):
    """include/sfk_resident.h sfk_pool_crop_desc: sfk_pool_desc plus the per-clip crop table (n, 2) = (top, left), or NULL,
    and RandomCrop's pad"""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("crop", C.c_void_p), ("fill", C.c_int32), ("pad", C.c_int32), ("out", C.c_void_p)]


class _PoolWarpDesc(C.Structure):
    """include/sfk_warp.h sfk_pool_warp_desc: sfk_pool_crop_desc with the per-clip matrix table (n, 6) float32 in place of crop
    and pad; index may be NULL (frame n*t + tt)"""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("warp", C.c_void_p), ("fill", C.c_int32), ("out", C.c_void_p)]


class _RoiPoolDesc(C.Structure):
    """include/sfk_roi_pool.h sfk_roi_pool_desc: sfk_roi_desc with its source addressing replaced by a frame pool -- byte
    (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch], clip n, time t reads frame index[n][t]"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("box", C.c_void_p), ("crop", C.c_void_p), ("pad", C.c_int32), ("fill", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("dst_dtype", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64),
                ("dt", C.c_int64), ("dc", C.c_int64), ("dh", C.c_int64), ("c_off", C.c_int32)]


class _RoiRaggedDesc(C.Structure):
    """include/sfk_roi_ragged.h sfk_roi_ragged_desc: sfk_roi_desc with its source addressing replaced by a byte arena -- frame
    t of clip n is hw[n] = (h_n, w_n) pixels of pixel_pitch packed bytes at arena + offset[n][t]"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("arena", C.c_void_p), ("arena_bytes", C.c_int64),
                ("pixel_pitch", C.c_int32), ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32),
                ("max_h", C.c_int32), ("max_w", C.c_int32), ("offset", C.c_void_p), ("hw", C.c_void_p), ("lut", C.c_void_p),
                ("box", C.c_void_p), ("crop", C.c_void_p), ("pad", C.c_int32), ("fill", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("dst_dtype", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64), ("dt", C.c_int64),
                ("dc", C.c_int64), ("dh", C.c_int64), ("c_off", C.c_int32)]


class _RoiWarpDesc(C.Structure):
    """include/sfk_roi_warp.h sfk_roi_warp_desc: sfk_roi_desc with the per-clip matrix table (n, 6) float32 in place of crop and
    pad"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("src", C.c_void_p), ("sn", C.c_int64),
                ("st", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("sc", C.c_int64), ("n", C.c_int32),
                ("t", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("lut", C.c_void_p), ("box", C.c_void_p), ("warp", C.c_void_p),
                ("dst_dtype", C.c_int32), ("reserved0", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64), ("dt", C.c_int64),
                ("dc", C.c_int64), ("dh", C.c_int64), ("c_off", C.c_int32), ("reserved1", C.c_int32)]


class _RoiPoolWarpDesc(C.Structure):
    """include/sfk_roi_warp.h sfk_roi_pool_warp_desc: sfk_roi_pool_desc with warp (n, 6) float32 in place of crop and pad"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("pool", C.c_void_p), ("frame_stride", C.c_int64),
                ("row_stride", C.c_int64), ("pixel_pitch", C.c_int32), ("frames", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32), ("index", C.c_void_p),
                ("lut", C.c_void_p), ("box", C.c_void_p), ("warp", C.c_void_p), ("fill", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("dst_dtype", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64),
                ("dt", C.c_int64), ("dc", C.c_int64), ("dh", C.c_int64), ("c_off", C.c_int32)]


class _RoiRaggedWarpDesc(C.Structure):
    """include/sfk_roi_warp.h sfk_roi_ragged_warp_desc: sfk_roi_ragged_desc with warp (n, 6) float32 in place of crop and pad"""
    _fields_ = [("struct_size", C.c_uint32), ("antialias", C.c_int32), ("arena", C.c_void_p), ("arena_bytes", C.c_int64),
                ("pixel_pitch", C.c_int32), ("c0", C.c_int32), ("c", C.c_int32), ("n", C.c_int32), ("t", C.c_int32),
                ("max_h", C.c_int32), ("max_w", C.c_int32), ("offset", C.c_void_p), ("hw", C.c_void_p), ("lut", C.c_void_p),
                ("box", C.c_void_p), ("warp", C.c_void_p), ("fill", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("dst_dtype", C.c_int32), ("dst", C.c_void_p), ("dn", C.c_int64), ("dt", C.c_int64),
                ("dc", C.c_int64), ("dh", C.c_int64), ("c_off", C.c_int32)]


class _ResizeDesc(C.Structure):
    """include/sfk_resize.h sfk_resize_desc: frame f is the contiguous HWC bytes src[offset[f] ...] of hw[f] = (h, w) pixels
    and c channels; its padded, cubic-resized (size, size, c) frame lands at out + f*out_frame_stride"""
    _fields_ = [("struct_size", C.c_uint32), ("fill", C.c_int32), ("src", C.c_void_p), ("src_bytes", C.c_int64),
                ("offset", C.c_void_p), ("hw", C.c_void_p), ("frames", C.c_int32), ("c", C.c_int32), ("size", C.c_int32),
                ("max_side", C.c_int32), ("out", C.c_void_p), ("out_frame_stride", C.c_int64)]


class _Tuning(C.Structure):
    """sfk_tuning: the write-once kernel-selection table of sfk_init (defaults = the measured best)."""
    _fields_ = [("struct_size", C.c_uint32), ("igemm_short_k", C.c_int32), ("igemm_small_k", C.c_int32), ("igemm_wide_store", C.c_int32),
                ("wgrad_target_8w", C.c_int32), ("wgrad_target_4w", C.c_int32), ("wgrad_use_workspace", C.c_int32),
                ("wgrad_wide_co", C.c_int32), ("bn_parts", C.c_int32), ("nt_apply_mb", C.c_int32),
                ("nt_reduce_mb", C.c_int32), ("nt_bwd_apply_mb", C.c_int32), ("igemm_pw_stream", C.c_int32),
                ("pool_blocks", C.c_int64), ("igemm_tile256", C.c_int32), ("wgrad_target_gen", C.c_int32),
                ("igemm_p8", C.c_int32), ("wgrad_p8", C.c_int32), ("igemm_halo", C.c_int32), ("wgrad_band", C.c_int32),
                ("stem_v3", C.c_int32)]


# experiment knobs (tools/gpu_ab_env.sh): read HERE, once, on the host side of the boundary -- the library itself never
# reads the environment (include/sfk.h); name -> sfk_tuning field
TUNING_ENV = {"SFK_KSHORT": "igemm_short_k", "SFK_SMALLK": "igemm_small_k", "SFK_WIDE": "igemm_wide_store",
              "SFK_WGT8": "wgrad_target_8w", "SFK_WGT4": "wgrad_target_4w", "SFK_WGWS_LIB": "wgrad_use_workspace",
              "SFK_WG_WIDECO": "wgrad_wide_co", "SFK_BN_PARTS": "bn_parts", "SFK_NT_APPLY_MB": "nt_apply_mb",
              "SFK_NT_RED_MB": "nt_reduce_mb", "SFK_NT_BAPP_MB": "nt_bwd_apply_mb", "SFK_POOL_BLOCKS": "pool_blocks",
              "SFK_PW_STREAM": "igemm_pw_stream", "SFK_TILE256": "igemm_tile256", "SFK_WGTG": "wgrad_target_gen",
              "SFK_P8": "igemm_p8",
              "SFK_WGP8": "wgrad_p8", "SFK_HALO": "igemm_halo", "SFK_WGBAND": "wgrad_band", "SFK_STEM3": "stem_v3"}

_PF, _PV, _I32, _I64, _F = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float
_P_FMAP = C.POINTER(_FMap)

# name -> argument types (return type is int unless listed in _RESTYPE)
SIGNATURES = {
    "sfk_conv_igemm": [C.POINTER(_ConvDesc), _PV],
    "sfk_conv_igemm_mtiles": [C.POINTER(_ConvDesc)],
    "sfk_conv_bnb_supported": [C.POINTER(_ConvDesc)],
    "sfk_conv_relu_out_supported": [C.POINTER(_ConvDesc)],
    "sfk_conv_epilogue_supported": [C.POINTER(_ConvDesc)],
    "sfk_conv_igemm_family": [C.POINTER(_ConvDesc)],
    "sfk_conv_igemm_route": [C.POINTER(_ConvDesc)],
    "sfk_bn_tail_fwd": [_PF, _PF, _I32, _I64, _PF, _I32, _PV, _I32, _I32, _PF, _PF, _F, _F, _PF, _PF, _PV, _PF, _PF, _PF, _PF, _PF, _PV, _PV],
    "sfk_bn_tail_bwd": [_PF, _PF, _I32, _PF, _I64, _PF, _I32, _PV, _I32, _I32, _PF, _PF, _PF, _PF, _PF, _PF, _PV, _PF, _PF, _PV],
    "sfk_conv_pw_dual_supported": [_P_FMAP, _P_FMAP, _P_FMAP],
    "sfk_conv_pw_dual": [_P_FMAP, _PV, _P_FMAP, _PV, _PF, _P_FMAP, _PV],
    "sfk_conv_wgrad": [C.POINTER(_WgradDesc), _PV],
    "sfk_conv_wgrad_workspace_bytes": [C.POINTER(_WgradDesc)],
    "sfk_conv_wgrad_dg_supported": [C.POINTER(_WgradDesc)],
    "sfk_conv_wgrad_wants_workspace": [C.POINTER(_WgradDesc)],
    "sfk_conv_wgrad_route": [C.POINTER(_WgradDesc)],
    "sfk_stem_kp": [_I32, _I32],
    "sfk_stem_conv_tiles": [C.POINTER(_StemSrc), _P_FMAP],
    "sfk_stem_conv_fwd": [C.POINTER(_StemSrc), _PV, _P_FMAP, _PF, _PV],
    "sfk_stem_conv_wgrad": [C.POINTER(_StemSrc), _P_FMAP, _PF, _PV],
    "sfk_stem_conv_fwd_route": [C.POINTER(_StemSrc), _P_FMAP],
    "sfk_stem_conv_wgrad_route": [C.POINTER(_StemSrc), _P_FMAP],
    "sfk_bn_finalize": [_PF, _I32, _I32, _I64, _PF, _PF, _F, _F, _PF, _PF, _PV, _PF, _PF, _PF, _PF, _PF, _PV],
    "sfk_bn_eval_coeffs": [_PF, _PF, _PF, _PF, _F, _I32, _PF, _PF, _PV],
    "sfk_bn_stats": [_P_FMAP, _PF, _I32, C.POINTER(C.c_int32), _PV],
    "sfk_bn_apply": [_P_FMAP, _PF, _PF, _P_FMAP, _PF, _PF, _I32, _P_FMAP, _PV, _PF, _I32, C.POINTER(C.c_int32), _PV],
    "sfk_bn_bwd_reduce": [_P_FMAP, _P_FMAP, _P_FMAP, _PF, _PF, _PF, _PF, _I32, _P_FMAP, _PF, _I32,
                          C.POINTER(C.c_int32), _PV, _PV],
    "sfk_bn_bwd_finalize": [_PF, _I32, _I32, _I64, _PF, _PF, _PF, _PF, _PF, _PF, _PV],
    "sfk_bn_bwd_apply": [_P_FMAP, _P_FMAP, _P_FMAP, _PF, _PF, _PF, _PF, _I32, _PF, _P_FMAP, _PV],
    "sfk_maxpool_fwd": [_P_FMAP, _P_FMAP, _PV, _I32, _I32, _I32, _PV],
    "sfk_maxpool_bwd": [_P_FMAP, _PV, _P_FMAP, _I32, _I32, _I32, _PV],
    "sfk_bn_maxpool_fwd": [_P_FMAP, _PF, _PF, _P_FMAP, _PV, _I32, _I32, _I32, _PV],
    "sfk_bn_maxpool_bwd_reduce": [_P_FMAP, _PV, _P_FMAP, _PF, _PF, _PF, _PF, _PF, _I32, C.POINTER(C.c_int32), _PV],
    "sfk_bn_maxpool_bwd_apply": [_P_FMAP, _PV, _P_FMAP, _PF, _PF, _PF, _PF, _PF, _P_FMAP, _PV],
    "sfk_head_pool_fwd": [_P_FMAP, _I32, _I32, _I32, _F, _PV, _PF, _I32, _I32, _PV],
    "sfk_head_pool_bwd": [_PF, _I32, _I32, _I32, _I32, _I32, _F, _PV, _P_FMAP, _PV],
    "sfk_head_dropout_mask": [_I32, _I32, _I32, _I32, _F, _PV, _PV, _PV],
    "sfk_fc_fwd": [_PF, _PF, _PF, _PF, _I32, _I32, _I32, _PV],
    "sfk_fc_bwd": [_PF, _PF, _PF, _PF, _PF, _PF, _I32, _I32, _I32, _PV],
    "sfk_softmax_ce": [_PF, _PV, _I32, _I32, _F, _PF, _PF, _PF, _PV, _PV],
    "sfk_adam": [_PF, _PF, _PF, _PF, _I64, _F, _F, _F, _F, _F, _PV, _PV, _I32, _PV],
    "sfk_filter_transpose": [_PV, _I32, _PV, _I32, _I32, _I32, _I32, _PV],
    "sfk_cast": [_PV, _I32, _PV, _I32, _I64, _PV],
    "sfk_fill_zero": [_PV, C.c_size_t, _PV],
    "sfk_u8_normalize_crop": [_PV, _PF, _PV, _I32, _PV, _I32, _I32, _I32, _I32, _I32, _I32, _PV],
    "sfk_eval_aggregate": [_PF, _PV, _PV, _I32, _I32, _I32, _PF, _PV, _PV, _PV],
    "sfk_sparse_fusion_fwd": [_PF, _PF, _PF, _PF, _I32, _I32, _I32, _PV],
    "sfk_sparse_fusion_bwd": [_PF, _PF, _PF, _PF, _I32, _I32, _I32, _PV],
    "sfk_filter_refresh": [_PF, _PV, _PV, _I32, _PV, _I32, _I32, _PV],
    "sfk_default_tuning": [C.POINTER(_Tuning)],
    "sfk_get_tuning": [C.POINTER(_Tuning)],
    "sfk_init": [C.POINTER(_Tuning)],
    "sfk_abi_version": [],
    "sfk_status_string": [C.c_int],
}
# include/sfk_stem2d.h: the frames-as-channels stem of the res2d model, same library, its own header and version
STEM2D_ABI_VERSION = 1     # include/sfk_stem2d.h SFK_STEM2D_ABI_VERSION
SIGNATURES_STEM2D = {
    "sfk_stem2d_abi_version": [],
    "sfk_stem2d_tiles": [C.POINTER(_Stem2dSrc), _P_FMAP],
    "sfk_stem2d_fwd": [C.POINTER(_Stem2dSrc), _PV, _P_FMAP, _PF, _PV],
    "sfk_stem2d_wgrad": [C.POINTER(_Stem2dSrc), _P_FMAP, _PF, _PV],
}
# include/sfk_u8stem.h: the stems reading uint8 frames through a table (MODEL.U8_STEM), same library, its own header and version
U8STEM_ABI_VERSION = 1     # include/sfk_u8stem.h SFK_U8STEM_ABI_VERSION
SIGNATURES_U8STEM = {
    "sfk_u8stem_abi_version": [],
    "sfk_u8stem_conv_fwd": [C.POINTER(_U8Clip), _PV, _I32, _I32, _PV, _P_FMAP, _PF, _PV],
    "sfk_u8stem_conv_wgrad": [C.POINTER(_U8Clip), _PV, _I32, _I32, _P_FMAP, _PF, _PV],
    "sfk_u8stem2d_fwd": [C.POINTER(_U8Clip), _PV, _P_FMAP, _PF, _PV],
    "sfk_u8stem2d_wgrad": [C.POINTER(_U8Clip), _P_FMAP, _PF, _PV],
}
# include/sfk_v2.h: the v2 part-box trainer's ROI crop-resize and SGD, same library, its own header and version
V2_ABI_VERSION = 1         # include/sfk_v2.h SFK_V2_ABI_VERSION
ROI_MAX_RATIO = 8          # include/sfk_v2.h SFK_ROI_MAX_RATIO
ROI_MAX_C = 16             # include/sfk_v2.h SFK_ROI_MAX_C
SIGNATURES_V2 = {
    "sfk_v2_abi_version": [],
    "sfk_roi_resize": [C.POINTER(_RoiDesc), _PV],
    "sfk_sgd": [_PF, _PF, _PF, _I64, C.c_float, C.c_float, C.c_float, _I32, C.c_float, _PV, _PV, _I32, _PV],
}
# include/sfk_aug.h: the device-side ColorJitter of the training clips, same library, its own header and version
AUG_ABI_VERSION = 1        # include/sfk_aug.h SFK_AUG_ABI_VERSION
SIGNATURES_AUG = {
    "sfk_aug_abi_version": [],
    "sfk_color_jitter_workspace_bytes": [_I32, _I32, _I32, _I32],
    "sfk_color_jitter": [C.POINTER(_JitterDesc), _PV],
}
# include/sfk_pool.h: the pooled evaluation input (one upload per test frame, windows gathered on the device), same library,
# its own header and version
POOL_ABI_VERSION = 1       # include/sfk_pool.h SFK_POOL_ABI_VERSION
POOL_MAX_ROW_BYTES = 60 * 1024   # include/sfk_pool.h SFK_POOL_MAX_ROW_BYTES
SIGNATURES_POOL = {
    "sfk_pool_abi_version": [],
    "sfk_u8_pool_gather": [C.POINTER(_PoolDesc), _PV],
}
# include/sfk_resize.h: the v1 loader's pad + bicubic resize of ragged crops on the device, same library, its own header and
# version
RESIZE_ABI_VERSION = 1     # include/sfk_resize.h SFK_RESIZE_ABI_VERSION
RESIZE_MAX_LDS_BYTES = 128 * 1024   # include/sfk_resize.h SFK_RESIZE_MAX_LDS_BYTES


def resize_lds_bytes(max_side: int, c: int, size: int) -> int:
    """include/sfk_resize.h SFK_RESIZE_LDS_BYTES: the LDS one workgroup of sfk_u8_pad_resize_cubic needs"""
    row16 = lambda b: (b + 30) // 16 * 16
    return max_side * ((c + 3) // 4) * 16 + 4 * (row16(max_side * c) + 16) + row16(size * c) + size * 36


SIGNATURES_RESIZE = {
    "sfk_resize_abi_version": [],
    "sfk_u8_pad_resize_cubic": [C.POINTER(_ResizeDesc), _PV],
}
# include/sfk_resident.h: the device-resident train set (cropped clips gathered from the frame pool), same library, its own
# header and version
RESIDENT_ABI_VERSION = 1   # include/sfk_resident.h SFK_RESIDENT_ABI_VERSION
SIGNATURES_RESIDENT = {
    "sfk_resident_abi_version": [],
    "sfk_u8_pool_gather_crop": [C.POINTER(_PoolCropDesc), _PV],
}
# include/sfk_roi_pool.h: the v2 trainer's device-resident train set (ROI crop-resize from the frame pool), same library, its
# own header and version
ROI_POOL_ABI_VERSION = 1   # include/sfk_roi_pool.h SFK_ROI_POOL_ABI_VERSION
SIGNATURES_ROI_POOL = {
    "sfk_roi_pool_abi_version": [],
    "sfk_roi_resize_pool": [C.POINTER(_RoiPoolDesc), _PV],
}
# include/sfk_roi_ragged.h: the v2 trainer's box-cropped resident train set (ROI crop-resize from a byte arena of ragged
# frames), same library, its own header and version
ROI_RAGGED_ABI_VERSION = 1   # include/sfk_roi_ragged.h SFK_ROI_RAGGED_ABI_VERSION
SIGNATURES_ROI_RAGGED = {
    "sfk_roi_ragged_abi_version": [],
    "sfk_roi_resize_ragged": [C.POINTER(_RoiRaggedDesc), _PV],
}
# include/sfk_u8stem_pool.h: the uint8 stems reading the frame pool through its index table (MODEL.POOL_STEM), same library, its
# own header and version
U8STEM_POOL_ABI_VERSION = 1   # include/sfk_u8stem_pool.h SFK_U8STEM_POOL_ABI_VERSION
SIGNATURES_U8STEM_POOL = {
    "sfk_u8stem_pool_abi_version": [],
    "sfk_u8pstem_conv_fwd": [C.POINTER(_U8PoolClip), _PV, _I32, _I32, _PV, _P_FMAP, _PF, _PV],
    "sfk_u8pstem_conv_wgrad": [C.POINTER(_U8PoolClip), _PV, _I32, _I32, _P_FMAP, _PF, _PV],
    "sfk_u8pstem2d_fwd": [C.POINTER(_U8PoolClip), _PV, _P_FMAP, _PF, _PV],
    "sfk_u8pstem2d_wgrad": [C.POINTER(_U8PoolClip), _P_FMAP, _PF, _PV],
}
# include/sfk_optim.h: the optimizer step with a device learning-rate table, weight decay and gradient clipping, same library,
# its own header and version
OPTIM_ABI_VERSION = 1      # include/sfk_optim.h SFK_OPTIM_ABI_VERSION
DECAY_MODES = {"none": 0, "l2": 1, "decoupled": 2}   # include/sfk_optim.h SFK_DECAY_*
GRAD_NORM_MAX_PARTS = 2048   # include/sfk_optim.h SFK_GRAD_NORM_MAX_PARTS
SIGNATURES_OPTIM = {
    "sfk_optim_abi_version": [],
    "sfk_adam_hp": [_PF, _PF, _PF, _PF, _I64, C.POINTER(_OptimHp), _F, _F, _F, _F, _PV, _PV, _I32, _PV],
    "sfk_sgd_hp": [_PF, _PF, _PF, _I64, C.POINTER(_OptimHp), _F, _F, _I32, _F, _PV, _PV, _I32, _PV],
    "sfk_grad_norm_parts": [_I64],
    "sfk_grad_norm": [_PF, _I64, _F, _F, _PV, _PF, _PV],
}
# include/sfk_groups.h: the optimizer step and the gradient norm over parameter groups and frozen ranges
GROUPS_ABI_VERSION = 1     # include/sfk_groups.h SFK_GROUPS_ABI_VERSION
GROUPS_MAX_SEGS, GROUPS_MAX_GROUPS = 2048, 64   # include/sfk_groups.h SFK_GROUPS_MAX_*
SIGNATURES_GROUPS = {
    "sfk_groups_abi_version": [],
    "sfk_groups_prepare": [_PV, _I32, _I64, _I32],
    "sfk_adam_groups": [_PF, _PF, _PF, _PF, _I64, C.POINTER(_GroupsHp), _F, _F, _F, _F, _PV, _PV, _I32, _PV],
    "sfk_sgd_groups": [_PF, _PF, _PF, _I64, C.POINTER(_GroupsHp), _F, _F, _I32, _F, _PV, _PV, _I32, _PV],
    "sfk_grad_norm_groups": [_PF, _I64, _PV, _PV, _I32, _F, _F, _PV, _PF, _PV],
}
# include/sfk_mix.h: Mixup / CutMix of the float clip in place and the soft-target loss, same library, its own header and version
MIX_ABI_VERSION = 1        # include/sfk_mix.h SFK_MIX_ABI_VERSION
MIX_ROW_FLOATS = 8         # include/sfk_mix.h SFK_MIX_ROW_FLOATS: partner, lam, y0, x0, y1, x1, weight, reserved
SIGNATURES_MIX = {
    "sfk_mix_abi_version": [],
    "sfk_clip_mix": [C.POINTER(_MixDesc), _PV],
    "sfk_softmax_ce_mix": [_PF, _PV, _PF, _F, _I32, _I32, _F, _PF, _PF, _PF, _PV, _PV],
}
# include/sfk_ema.h: the exponential moving average of the weights and the exchange that evaluates it, same library, its own
# header and version
EMA_ABI_VERSION = 1        # include/sfk_ema.h SFK_EMA_ABI_VERSION
EMA_MAX_TENSORS = 4096     # include/sfk_ema.h SFK_EMA_MAX_TENSORS
SIGNATURES_EMA = {
    "sfk_ema_abi_version": [],
    "sfk_ema_update": [C.POINTER(_EmaDesc), _PV],
    "sfk_ema_swap": [C.POINTER(_EmaDesc), _PV],
}
# include/sfk_warp.h: the per-clip affine sampling of the frame pool (rotate, scale, shear, flip), same library, its own header
# and version
WARP_ABI_VERSION = 1       # include/sfk_warp.h SFK_WARP_ABI_VERSION
WARP_TILE_H, WARP_TILE_W = 16, 32      # include/sfk_warp.h SFK_WARP_TILE_H / _W: the output tile of one workgroup
WARP_LDS_BYTES = 32 * 1024             # include/sfk_warp.h SFK_WARP_LDS_BYTES
WARP_ROW_FLOATS = 6        # (a, b, c, d, e, f): output pixel (x, y) reads source (a x + b y + c, d x + e y + f)
SIGNATURES_WARP = {
    "sfk_warp_abi_version": [],
    "sfk_u8_pool_gather_warp": [C.POINTER(_PoolWarpDesc), _PV],
    "sfk_warp_fallback_tiles": [_I32, _I32, _I32, _I32, _PF],
}
# include/sfk_roi_warp.h: the v2 part-box resize sampled through a per-clip affine matrix (the three sources of sfk_roi_resize*),
# same library, its own header and version
ROI_WARP_ABI_VERSION = 1   # include/sfk_roi_warp.h SFK_ROI_WARP_ABI_VERSION
ROI_WARP_TILE_H, ROI_WARP_TILE_W = 16, 32   # include/sfk_roi_warp.h SFK_ROI_WARP_TILE_H / _W: the output tile of one workgroup
ROI_WARP_LDS_BYTES = 24 * 1024              # include/sfk_roi_warp.h SFK_ROI_WARP_LDS_BYTES
SIGNATURES_ROI_WARP = {
    "sfk_roi_warp_abi_version": [],
    "sfk_roi_resize_warp": [C.POINTER(_RoiWarpDesc), _PV],
    "sfk_roi_resize_pool_warp": [C.POINTER(_RoiPoolWarpDesc), _PV],
    "sfk_roi_resize_ragged_warp": [C.POINTER(_RoiRaggedWarpDesc), _PV],
}
_RESTYPE = {"sfk_status_string": C.c_char_p, "sfk_conv_wgrad_route": C.c_int64, "sfk_stem_conv_fwd_route": C.c_int64, "sfk_stem_conv_wgrad_route": C.c_int64, "sfk_groups_prepare": C.c_int64, "sfk_conv_wgrad_workspace_bytes": C.c_int64,
            "sfk_color_jitter_workspace_bytes": C.c_int64}


def new_conv_desc() -> "_ConvDesc":
    """a zeroed sfk_conv_desc carrying the ABI handshake (struct_size = the layout THIS binding was written for)"""
    d = _ConvDesc()
    d.struct_size = C.sizeof(_ConvDesc)
    return d


def new_wgrad_desc() -> "_WgradDesc":
    d = _WgradDesc()
    d.struct_size = C.sizeof(_WgradDesc)
    return d


def new_stem2d_src() -> "_Stem2dSrc":
    d = _Stem2dSrc()
    d.struct_size = C.sizeof(_Stem2dSrc)
    return d


def new_u8_clip() -> "_U8Clip":
    d = _U8Clip()
    d.struct_size = C.sizeof(_U8Clip)
    return d


def new_u8_pool_clip() -> "_U8PoolClip":
    d = _U8PoolClip()
    d.struct_size = C.sizeof(_U8PoolClip)
    return d


def new_roi_desc() -> "_RoiDesc":
    d = _RoiDesc()
    d.struct_size = C.sizeof(_RoiDesc)
    return d


def new_jitter_desc() -> "_JitterDesc":
    d = _JitterDesc()
    d.struct_size = C.sizeof(_JitterDesc)
    return d


def new_mix_desc() -> "_MixDesc":
    d = _MixDesc()
    d.struct_size = C.sizeof(_MixDesc)
    return d


def new_ema_desc() -> "_EmaDesc":
    d = _EmaDesc()
    d.struct_size = C.sizeof(_EmaDesc)
    return d


class EmaTable:
    """The table of include/sfk_ema.h, ready to launch: the (src, dst) tensors it points into, kept alive, and its device
    copy (None when it has no entry).  Built once (HipBackend.ema_table) and shared by the update and the swap."""

    def __init__(self, pairs, dev):
        self.pairs, self.dev = pairs, dev

    @property
    def ntensors(self) -> int:
        return len(self.pairs)


def new_pool_desc() -> "_PoolDesc":
    d = _PoolDesc()
    d.struct_size = C.sizeof(_PoolDesc)
    return d


def new_pool_crop_desc() -> "_PoolCropDesc":
    d = _PoolCropDesc()
    d.struct_size = C.sizeof(_PoolCropDesc)
    return d


def new_pool_warp_desc() -> "_PoolWarpDesc":
    d = _PoolWarpDesc()
    d.struct_size = C.sizeof(_PoolWarpDesc)
    return d


def new_roi_pool_desc() -> "_RoiPoolDesc":
    d = _RoiPoolDesc()
    d.struct_size = C.sizeof(_RoiPoolDesc)
    return d


def new_roi_ragged_desc() -> "_RoiRaggedDesc":
    d = _RoiRaggedDesc()
    d.struct_size = C.sizeof(_RoiRaggedDesc)
    return d


def new_roi_warp_desc() -> "_RoiWarpDesc":
    d = _RoiWarpDesc()
    d.struct_size = C.sizeof(_RoiWarpDesc)
    return d


def new_roi_pool_warp_desc() -> "_RoiPoolWarpDesc":
    d = _RoiPoolWarpDesc()
    d.struct_size = C.sizeof(_RoiPoolWarpDesc)
    return d


def new_roi_ragged_warp_desc() -> "_RoiRaggedWarpDesc":
    d = _RoiRaggedWarpDesc()
    d.struct_size = C.sizeof(_RoiRaggedWarpDesc)
    return d


def new_optim_hp() -> "_OptimHp":
    d = _OptimHp()
    d.struct_size = C.sizeof(_OptimHp)
    return d


class GroupTable:
    """A segment table of include/sfk_groups.h, ready to launch: the host mirror (a ctypes array with tile0 filled by
    sfk_groups_prepare), its device copy, and the per-group weight decays on the device.  Built once (HipBackend.group_table)
    and shared by the update and the norm launch that use it."""

    def __init__(self, segments, host, dev, wds, ngroups, count):
        self.segments, self.host, self.dev, self.wds, self.ngroups, self.count = segments, host, dev, wds, ngroups, count

    @property
    def nsegs(self) -> int:
        return len(self.segments)


def new_resize_desc() -> "_ResizeDesc":
    d = _ResizeDesc()
    d.struct_size = C.sizeof(_ResizeDesc)
    return d


def new_tuning() -> "_Tuning":
    t = _Tuning()
    t.struct_size = C.sizeof(_Tuning)
    return t

_lib = None


def load(path: str = LIB_PATH) -> C.CDLL:
    """dlopen libsfk.so and type every entry point of include/sfk.h.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SfkError(f"{path} not found: build it with `python video-classification_amd/build.py` "
                       "(there is no CPU or PyTorch fallback for the SlowFast path)")
    lib = C.CDLL(path)
    for table in (SIGNATURES, SIGNATURES_STEM2D, SIGNATURES_U8STEM, SIGNATURES_V2, SIGNATURES_AUG, SIGNATURES_POOL,
                  SIGNATURES_RESIZE, SIGNATURES_RESIDENT, SIGNATURES_ROI_POOL, SIGNATURES_ROI_RAGGED, SIGNATURES_U8STEM_POOL,
                  SIGNATURES_OPTIM, SIGNATURES_GROUPS, SIGNATURES_MIX, SIGNATURES_EMA, SIGNATURES_WARP, SIGNATURES_ROI_WARP):
        for name, argtypes in table.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.argtypes = argtypes
            fn.restype = _RESTYPE[name] if name in _RESTYPE else C.c_int
    if lib.sfk_abi_version() != ABI_VERSION:
        raise SfkError(f"libsfk ABI version mismatch: library {lib.sfk_abi_version()}, binding {ABI_VERSION}")
    if lib.sfk_stem2d_abi_version() != STEM2D_ABI_VERSION:
        raise SfkError(f"libsfk stem2d ABI version mismatch: library {lib.sfk_stem2d_abi_version()}, binding {STEM2D_ABI_VERSION}")
    if lib.sfk_u8stem_abi_version() != U8STEM_ABI_VERSION:
        raise SfkError(f"libsfk u8stem ABI version mismatch: library {lib.sfk_u8stem_abi_version()}, binding {U8STEM_ABI_VERSION}")
    if lib.sfk_v2_abi_version() != V2_ABI_VERSION:
        raise SfkError(f"libsfk v2 ABI version mismatch: library {lib.sfk_v2_abi_version()}, binding {V2_ABI_VERSION}")
    if lib.sfk_aug_abi_version() != AUG_ABI_VERSION:
        raise SfkError(f"libsfk aug ABI version mismatch: library {lib.sfk_aug_abi_version()}, binding {AUG_ABI_VERSION}")
    if lib.sfk_pool_abi_version() != POOL_ABI_VERSION:
        raise SfkError(f"libsfk pool ABI version mismatch: library {lib.sfk_pool_abi_version()}, binding {POOL_ABI_VERSION}")
    if lib.sfk_resize_abi_version() != RESIZE_ABI_VERSION:
        raise SfkError(f"libsfk resize ABI version mismatch: library {lib.sfk_resize_abi_version()}, binding {RESIZE_ABI_VERSION}")
    if lib.sfk_resident_abi_version() != RESIDENT_ABI_VERSION:
        raise SfkError(f"libsfk resident ABI version mismatch: library {lib.sfk_resident_abi_version()}, binding {RESIDENT_ABI_VERSION}")
    if lib.sfk_roi_pool_abi_version() != ROI_POOL_ABI_VERSION:
        raise SfkError(f"libsfk roi_pool ABI version mismatch: library {lib.sfk_roi_pool_abi_version()}, binding {ROI_POOL_ABI_VERSION}")
    if lib.sfk_roi_ragged_abi_version() != ROI_RAGGED_ABI_VERSION:
        raise SfkError(f"libsfk roi_ragged ABI version mismatch: library {lib.sfk_roi_ragged_abi_version()}, binding {ROI_RAGGED_ABI_VERSION}")
    if lib.sfk_u8stem_pool_abi_version() != U8STEM_POOL_ABI_VERSION:
        raise SfkError(f"libsfk u8stem_pool ABI version mismatch: library {lib.sfk_u8stem_pool_abi_version()}, binding {U8STEM_POOL_ABI_VERSION}")
    if lib.sfk_optim_abi_version() != OPTIM_ABI_VERSION:
        raise SfkError(f"libsfk optim ABI version mismatch: library {lib.sfk_optim_abi_version()}, binding {OPTIM_ABI_VERSION}")
    if lib.sfk_groups_abi_version() != GROUPS_ABI_VERSION:
        raise SfkError(f"libsfk groups ABI version mismatch: library {lib.sfk_groups_abi_version()}, binding {GROUPS_ABI_VERSION}")
    if lib.sfk_mix_abi_version() != MIX_ABI_VERSION:
        raise SfkError(f"libsfk mix ABI version mismatch: library {lib.sfk_mix_abi_version()}, binding {MIX_ABI_VERSION}")
    if lib.sfk_ema_abi_version() != EMA_ABI_VERSION:
        raise SfkError(f"libsfk ema ABI version mismatch: library {lib.sfk_ema_abi_version()}, binding {EMA_ABI_VERSION}")
    if lib.sfk_warp_abi_version() != WARP_ABI_VERSION:
        raise SfkError(f"libsfk warp ABI version mismatch: library {lib.sfk_warp_abi_version()}, binding {WARP_ABI_VERSION}")
    if lib.sfk_roi_warp_abi_version() != ROI_WARP_ABI_VERSION:
        raise SfkError(f"libsfk roi_warp ABI version mismatch: library {lib.sfk_roi_warp_abi_version()}, binding {ROI_WARP_ABI_VERSION}")
    t = new_tuning()
    if lib.sfk_default_tuning(C.byref(t)) != 0:
        raise SfkError("sfk_default_tuning refused this binding's sfk_tuning layout")
    for env, fld in TUNING_ENV.items():
        if os.environ.get(env) is not None:
            setattr(t, fld, int(os.environ[env]))
    st = lib.sfk_init(C.byref(t))                # once per process, before the first launch
    if st != 0:
        raise SfkError(f"sfk_init: {lib.sfk_status_string(st).decode()}")
    _lib = lib
    return lib


def tuning() -> _Tuning:
    """the table the loaded library runs with (sfk_get_tuning)"""
    t = new_tuning()
    _check(load().sfk_get_tuning(C.byref(t)), "sfk_get_tuning")
    return t


def _check(st: int, what: str):
    if st != 0:
        msg = load().sfk_status_string(st).decode()
        raise SfkError(f"{what}: {msg} ({st})")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _c_fmap(f: FMap) -> _FMap:
    return _FMap(f.buf.data_ptr(), _DT[f.buf.dtype], f.n, f.t, f.h, f.w, f.c, f.ld, f.c_off)


def _c_taps(taps: Sequence[Tap]):
    arr = (_Tap * SFK_MAX_TAPS)()
    assert 0 < len(taps) <= SFK_MAX_TAPS
    for i, (dt, dh, dw, wi) in enumerate(taps):
        arr[i] = _Tap(dt, dh, dw, wi)
    return arr


def _c_conv(p: ConvPass) -> _ConvDesc:
    d = new_conv_desc()
    d.x, d.y = _c_fmap(p.x), _c_fmap(p.y)
    d.rt, d.rh, d.rw = p.rows
    d.gs = (C.c_int32 * 3)(*p.gs)
    d.os = (C.c_int32 * 3)(*p.os)
    d.oo = (C.c_int32 * 3)(*p.oo)
    d.ntaps = len(p.taps)
    d.taps = _c_taps(p.taps)
    d.w = p.w.data_ptr()
    d.wtaps, d.cin, d.cout = p.wtaps, p.cin, p.cout
    d.accumulate = 1 if p.accumulate else 0
    d.stats = _ptr(p.stats)
    if p.bnb is not None:
        b = p.bnb
        if b.y_bn is not None:
            d.bnb.y_bn = _c_fmap(b.y_bn)
        if b.mask_src is not None:
            d.bnb.mask_src = _c_fmap(b.mask_src)
        d.bnb.mean, d.bnb.invstd = _ptr(b.mean), _ptr(b.invstd)
        d.bnb.scale, d.bnb.shift = _ptr(b.scale), _ptr(b.shift)
        d.bnb.relu = 1 if b.relu else 0
        d.bnb.partials = _ptr(b.partials)
    if p.relu_out_bits is not None:
        vec = 8 if p.y.dtype == torch.bfloat16 else 4
        assert p.relu_out_bits.dtype == torch.uint8 and p.relu_out_bits.numel() >= p.y.pixels * (p.cout // vec)
        d.out_relu_bits = p.relu_out_bits.data_ptr()
    if p.ep is not None:
        e = p.ep
        assert e.scale is not None or e.shift is not None
        d.ep.scale, d.ep.shift = _ptr(e.scale), _ptr(e.shift)
        if e.res is not None:
            d.ep.res = _c_fmap(e.res)
        d.ep.res_scale, d.ep.res_shift = _ptr(e.res_scale), _ptr(e.res_shift)
        d.ep.relu = 1 if e.relu else 0
        if e.relu_bits is not None:
            vec = 8 if p.y.dtype == torch.bfloat16 else 4
            assert e.relu_bits.dtype == torch.uint8 and e.relu_bits.numel() >= p.y.pixels * (p.cout // vec)
            d.ep.relu_bits = e.relu_bits.data_ptr()
    return d


class HipBackend:
    """Every method returns ``run(stream)``; descriptors are built once, here.  Tensors referenced by a closure
    are kept alive by it."""

    name = "hip"

    def __init__(self):
        self.lib = load()

    # -- convolution
    def conv_igemm_mtiles(self, p: ConvPass) -> int:
        d = _c_conv(p)
        r = self.lib.sfk_conv_igemm_mtiles(C.byref(d))
        if r < 0:
            _check(r, "sfk_conv_igemm_mtiles")
        return r

    def conv_bnb_supported(self, p: ConvPass) -> bool:
        """can this pass take a BnBwdFuse (sfk_conv_bnb_supported)?"""
        return bool(self.lib.sfk_conv_bnb_supported(C.byref(_c_conv(p))))

    def conv_relu_out_supported(self, p: ConvPass) -> bool:
        """can this pass apply a ReLU bitmap to what it stores (sfk_conv_relu_out_supported)?"""
        q = ConvPass(**{**p.__dict__, "relu_out_bits": None})
        return bool(self.lib.sfk_conv_relu_out_supported(C.byref(_c_conv(q))))

    def conv_epilogue_supported(self, p: ConvPass) -> bool:
        """can this pass run with its fused output transform p.ep (sfk_conv_epilogue_supported)?"""
        return bool(self.lib.sfk_conv_epilogue_supported(C.byref(_c_conv(p))))

    def conv_family(self, p: ConvPass) -> int:
        """0 register-staged igemm, 1 LDS-DMA igemm, 3 streaming pointwise kernel with the fused epilogue, 4 the deep-pipelined
        256 x 256 tile (conv_igemm_p8.hip), 5 the LDS-band 3 x 3 kernel (conv_halo.hip)"""
        return int(self.lib.sfk_conv_igemm_family(C.byref(_c_conv(p))))

    def conv_route(self, p: ConvPass) -> int:
        """the kernel instantiation sfk_conv_igemm runs for p: an sfk_igemm_route of include/sfk.h (the launch code run dry)"""
        r = int(self.lib.sfk_conv_igemm_route(C.byref(_c_conv(p))))
        if r < 0:
            _check(r, "sfk_conv_igemm_route")
        return r

    def conv_igemm(self, p: ConvPass):
        d, fn, keep = _c_conv(p), self.lib.sfk_conv_igemm, p

        def run(stream, _d=C.byref(d), _keep=(d, keep)):
            st = fn(_d, stream)
            if st:
                _check(st, "sfk_conv_igemm")
        return run

    def _wgrad_desc(self, p: WgradPass):
        d = new_wgrad_desc()
        d.x, d.dy = _c_fmap(p.x), _c_fmap(p.dy)
        d.gs = (C.c_int32 * 3)(*p.gs)
        d.ntaps, d.taps = len(p.taps), _c_taps(p.taps)
        d.dw, d.wtaps, d.cin, d.cout = p.dw.data_ptr(), p.wtaps, p.cin, p.cout
        if p.dg_w is not None:
            d.dg_w, d.dg_y = p.dg_w.data_ptr(), _c_fmap(p.dg_y)
        return d

    def conv_wgrad_dg_supported(self, p: WgradPass) -> bool:
        """the fused data gradient (p.dg_w, p.dg_y) can run with this filter-gradient pass"""
        return p.dg_w is not None and bool(self.lib.sfk_conv_wgrad_dg_supported(C.byref(self._wgrad_desc(p))))

    def conv_wgrad_wants_workspace(self, p: WgradPass) -> bool:
        """this pass would run the 256-column tile, which sums its pixel splits only through a workspace"""
        return bool(self.lib.sfk_conv_wgrad_wants_workspace(C.byref(self._wgrad_desc(p))))

    def conv_wgrad_workspace_bytes(self, p: WgradPass) -> int:
        """bytes of scratch with which sfk_conv_wgrad sums its pixel splits without atomics (deterministically)"""
        r = self.lib.sfk_conv_wgrad_workspace_bytes(C.byref(self._wgrad_desc(p)))
        if r < 0:
            _check(int(r), "sfk_conv_wgrad_workspace_bytes")
        return int(r)

    def conv_wgrad_route(self, p: WgradPass) -> Tuple[int, bool, int]:
        """(sfk_wgrad_route of include/sfk.h, workspace path taken with p.workspace, pixel splits) of sfk_conv_wgrad(p)"""
        d = self._wgrad_desc(p)
        if p.workspace is not None:
            d.workspace, d.workspace_bytes = p.workspace.data_ptr(), p.workspace.numel() * p.workspace.element_size()
        r = int(self.lib.sfk_conv_wgrad_route(C.byref(d)))
        if r < 0:
            _check(r, "sfk_conv_wgrad_route")
        return r & 0x5FFFFFFF, bool((r >> 29) & 1), r >> 32     # (the id keeps bit 30: SFK_WGRAD_ROUTE_RING5)

    def conv_wgrad(self, p: WgradPass):
        d = self._wgrad_desc(p)
        if p.workspace is not None:
            d.workspace, d.workspace_bytes = p.workspace.data_ptr(), p.workspace.numel() * p.workspace.element_size()
        fn = self.lib.sfk_conv_wgrad

        def run(stream, _d=C.byref(d), _keep=(d, p)):
            st = fn(_d, stream)
            if st:
                _check(st, "sfk_conv_wgrad")
        return run

    @staticmethod
    def _c_stem(p: StemSrc) -> _StemSrc:
        s = p.src
        assert s.dim() == 5
        d = _StemSrc()
        d.src, d.src_dtype = s.data_ptr(), _DT[s.dtype]
        d.sn, d.sc, d.st, d.sh, d.sw = s.stride()
        d.cin, d.t_in, d.h_in, d.w_in = s.shape[1], s.shape[2], s.shape[3], s.shape[4]
        d.t_index = _ptr(p.t_index)
        d.t_len = p.t_len
        d.kt = p.kt
        return d

    def stem_conv_tiles(self, p: StemSrc, y: FMap) -> int:
        d, fy = self._c_stem(p), _c_fmap(y)
        r = self.lib.sfk_stem_conv_tiles(C.byref(d), C.byref(fy))
        if r < 0:
            _check(r, "sfk_stem_conv_tiles")
        return r

    def stem_conv_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        d, fy = self._c_stem(p), _c_fmap(y)
        return self._plain("sfk_stem_conv_fwd", C.byref(d), _ptr(w), C.byref(fy), _ptr(stats), keep=(d, fy, p, w, y, stats))

    def stem_conv_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        d, fy = self._c_stem(p), _c_fmap(dy)
        return self._plain("sfk_stem_conv_wgrad", C.byref(d), C.byref(fy), _ptr(dw), keep=(d, fy, p, dy, dw))

    def stem_route(self, p: StemSrc, m: FMap, wgrad: bool = False) -> Tuple[int, int, int]:
        """(sfk_stem_route of include/sfk.h, work items, workgroups / blocks) of sfk_stem_conv_fwd(p, ., m) or, with wgrad,
        of sfk_stem_conv_wgrad(p, m, .): the launch code run dry"""
        name = "sfk_stem_conv_wgrad_route" if wgrad else "sfk_stem_conv_fwd_route"
        d, fm = self._c_stem(p), _c_fmap(m)
        r = int(getattr(self.lib, name)(C.byref(d), C.byref(fm)))
        if r < 0:
            _check(r, name)
        return r & 0xFFFF, (r >> 36) & 0x7FFFFFF, (r >> 16) & 0xFFFFF

    # -- the frames-as-channels stem of res2d (include/sfk_stem2d.h); `src` of the StemSrc is indexed (n, c, t, h, w), kt = T
    @staticmethod
    def _c_stem2d(p: StemSrc) -> _Stem2dSrc:
        s = p.src
        assert s.dim() == 5 and p.t_index is None
        d = new_stem2d_src()
        d.src, d.src_dtype = s.data_ptr(), _DT[s.dtype]
        d.sn, d.sc, d.st, d.sh, d.sw = s.stride()
        d.n, d.c, d.t, d.h_in, d.w_in = s.shape
        return d

    def stem2d_tiles(self, p: StemSrc, y: FMap) -> int:
        d, fy = self._c_stem2d(p), _c_fmap(y)
        r = self.lib.sfk_stem2d_tiles(C.byref(d), C.byref(fy))
        if r < 0:
            _check(r, "sfk_stem2d_tiles")
        return r

    def stem2d_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        d, fy = self._c_stem2d(p), _c_fmap(y)
        return self._plain("sfk_stem2d_fwd", C.byref(d), _ptr(w), C.byref(fy), _ptr(stats), keep=(d, fy, p, w, y, stats))

    def stem2d_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        d, fy = self._c_stem2d(p), _c_fmap(dy)
        return self._plain("sfk_stem2d_wgrad", C.byref(d), C.byref(fy), _ptr(dw), keep=(d, fy, p, dy, dw))

    # -- the stems reading uint8 frames (include/sfk_u8stem.h); `src` of the StemSrc is an input_pipeline.U8Clip
    @staticmethod
    def _c_u8clip(p: StemSrc) -> _U8Clip:
        x = p.src
        f = x.frames
        assert f.dtype == torch.uint8 and f.dim() == 5 and f.stride(4) == 1
        d = new_u8_clip()
        d.src, d.lut, d.crop, d.pad = f.data_ptr(), x.lut.data_ptr(), _ptr(x.crop), x.pad
        d.sn, d.st, d.sh, d.sw = f.stride()[:4]
        d.c0, d.c = x.c0, x.c
        d.n, d.t, d.h, d.w = f.shape[:4]
        return d

    def u8stem_tiles(self, p: StemSrc, y: FMap) -> int:
        """the BatchNorm partial-sum rows of either u8 stem, over a U8Clip or a PoolClip alike: sfk_stem_conv_tiles' count,
        which depends on the output map only (for the one-frame output of the 2-D stem it equals sfk_stem2d_tiles')"""
        d, fy = _StemSrc(), _c_fmap(y)
        r = self.lib.sfk_stem_conv_tiles(C.byref(d), C.byref(fy))
        if r < 0:
            _check(r, "sfk_stem_conv_tiles")
        return r

    def _u8_stem_op(self, name: str, c_desc, temporal: bool, p: StemSrc, m: FMap, pre: tuple, post: tuple):
        """one uint8 stem entry point: name(descriptor, [t_index, t_len, kt,] *pre, map, *post, stream); c_desc builds the
        descriptor of p.src, the 2-D stems (not temporal) take no frame selection"""
        assert temporal or p.t_index is None
        d, fm = c_desc(p), _c_fmap(m)
        sel = (_ptr(p.t_index), p.t_len, p.kt) if temporal else ()
        return self._plain(name, C.byref(d), *sel, *map(_ptr, pre), C.byref(fm), *map(_ptr, post), keep=(d, fm, p, *pre, m, *post))

    def u8stem_conv_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        return self._u8_stem_op("sfk_u8stem_conv_fwd", self._c_u8clip, True, p, y, (w,), (stats,))

    def u8stem_conv_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        return self._u8_stem_op("sfk_u8stem_conv_wgrad", self._c_u8clip, True, p, dy, (), (dw,))

    def u8stem2d_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        return self._u8_stem_op("sfk_u8stem2d_fwd", self._c_u8clip, False, p, y, (w,), (stats,))

    def u8stem2d_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        return self._u8_stem_op("sfk_u8stem2d_wgrad", self._c_u8clip, False, p, dy, (), (dw,))

    # -- the uint8 stems reading the frame pool (include/sfk_u8stem_pool.h); `src` of the StemSrc is an input_pipeline.PoolClip
    #    (the BatchNorm partial-sum rows: u8stem_tiles, which reads the output map only)
    @staticmethod
    def _c_u8poolclip(p: StemSrc) -> _U8PoolClip:
        x = p.src
        a, idx = x.arena, x.index
        assert a.dtype == torch.uint8 and a.dim() == 4 and a.stride(3) == 1
        assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.is_contiguous()
        d = new_u8_pool_clip()
        d.pool, d.index, d.lut, d.crop = a.data_ptr(), idx.data_ptr(), x.lut.data_ptr(), _ptr(x.crop)
        d.frame_stride, d.row_stride, d.pixel_pitch = a.stride()[:3]
        d.frames, d.h, d.w = a.shape[:3]
        d.n, d.t = idx.shape
        d.c0, d.c, d.pad, d.fill = x.c0, x.c, x.pad, x.fill
        return d

    def u8pstem_conv_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        return self._u8_stem_op("sfk_u8pstem_conv_fwd", self._c_u8poolclip, True, p, y, (w,), (stats,))

    def u8pstem_conv_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        return self._u8_stem_op("sfk_u8pstem_conv_wgrad", self._c_u8poolclip, True, p, dy, (), (dw,))

    def u8pstem2d_fwd(self, p: StemSrc, w: torch.Tensor, y: FMap, stats: Optional[torch.Tensor]):
        return self._u8_stem_op("sfk_u8pstem2d_fwd", self._c_u8poolclip, False, p, y, (w,), (stats,))

    def u8pstem2d_wgrad(self, p: StemSrc, dy: FMap, dw: torch.Tensor):
        return self._u8_stem_op("sfk_u8pstem2d_wgrad", self._c_u8poolclip, False, p, dy, (), (dw,))

    # -- generic plain-argument entry points
    def _plain(self, name, *args, keep=()):
        fn = getattr(self.lib, name)
        cargs = tuple(args)

        def run(stream, _a=cargs, _keep=keep):
            st = fn(*_a, stream)
            if st:
                _check(st, name)
        run.sfk_name = name          # for the profiler's per-op dump
        return run

    def bn_finalize(self, partials, nparts, c, count, gamma, beta, eps, momentum, running_mean, running_var, nbt,
                    mean, invstd, scale, shift, workspace=None):
        """workspace: optional BN_FOLD_ROWS * c * 2 floats (parallel first-level fold of many partial rows)"""
        ts = (partials, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, workspace)
        return self._plain("sfk_bn_finalize", _ptr(partials), nparts, c, count, _ptr(gamma), _ptr(beta), eps, momentum,
                           _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(mean), _ptr(invstd), _ptr(scale),
                           _ptr(shift), _ptr(workspace), keep=ts)

    def bn_eval_coeffs(self, gamma, beta, rm, rv, eps, c, scale, shift):
        return self._plain("sfk_bn_eval_coeffs", _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), eps, c, _ptr(scale),
                           _ptr(shift), keep=(gamma, beta, rm, rv, scale, shift))

    def bn_stats(self, y: FMap, partials, max_parts):
        """returns (run, nparts)"""
        fy = _c_fmap(y)
        np_ = C.c_int32(0)
        run = self._plain("sfk_bn_stats", C.byref(fy), _ptr(partials), max_parts, C.byref(np_),
                          keep=(fy, np_, y, partials))
        return run, self._dry_parts(y, max_parts)

    @staticmethod
    def _dry_parts(y: FMap, max_parts: int) -> int:
        # mirrors chan_grid() in csrc/bn.hip
        vec = 8 if y.dtype == torch.bfloat16 else 4
        cgs = y.c // vec
        cgs_b = min(cgs, 256)
        rows_b = 256 // cgs_b
        parts = (y.pixels + rows_b * 16 - 1) // (rows_b * 16)
        cchunks = (cgs + 255) // 256
        parts = min(parts, max(1, int(tuning().bn_parts) // cchunks))
        if max_parts > 0:
            parts = min(parts, max_parts)
        return max(1, parts)

    def bn_apply(self, y: FMap, scale, shift, res: Optional[FMap], res_scale, res_shift, relu: bool, out: FMap,
                 relu_bits=None, out_sums=None, max_parts: int = 0):
        """relu_bits: optional uint8 tensor of pixels * c / V bytes (V = 8 bf16, 4 f32) that receives the ReLU mask.
        out_sums: optional fp32 [max_parts][c][2] that receives the partial column sums of the output; then the call returns
        (run, nparts) -- nparts is fixed by the geometry, the library reports it when the launch is configured"""
        fy, fo = _c_fmap(y), _c_fmap(out)
        fr = _c_fmap(res) if res is not None else None
        if relu_bits is not None:
            vec = 8 if y.dtype == torch.bfloat16 else 4
            assert relu_bits.dtype == torch.uint8 and relu_bits.numel() >= y.pixels * (y.c // vec)
        np_ = C.c_int32(0)
        if out_sums is not None:
            assert max_parts > 0 and out_sums.numel() >= max_parts * y.c * 2
        run = self._plain("sfk_bn_apply", C.byref(fy), _ptr(scale), _ptr(shift), C.byref(fr) if fr else None,
                          _ptr(res_scale), _ptr(res_shift), 1 if relu else 0, C.byref(fo), _ptr(relu_bits), _ptr(out_sums),
                          max_parts, C.byref(np_) if out_sums is not None else None,
                          keep=(fy, fo, fr, np_, y, out, res, scale, shift, res_scale, res_shift, relu_bits, out_sums))
        if out_sums is None:
            return run
        return run, self._dry_parts(y, max_parts)

    def bn_bwd_reduce(self, da: FMap, y: FMap, mask_src: Optional[FMap], mean, invstd, scale, shift, relu: bool,
                      dz_out: Optional[FMap], partials, max_parts, relu_bits=None):
        """returns (run, nparts); relu_bits: the mask bn_apply wrote (then mask_src must be None)."""
        if relu_bits is not None:
            vec = 8 if da.dtype == torch.bfloat16 else 4
            assert relu_bits.dtype == torch.uint8 and relu_bits.numel() >= da.pixels * (da.c // vec)
        fa, fy = _c_fmap(da), (_c_fmap(y) if y is not None else None)
        fm = _c_fmap(mask_src) if mask_src is not None else None
        fz = _c_fmap(dz_out) if dz_out is not None else None
        np_ = C.c_int32(0)
        run = self._plain("sfk_bn_bwd_reduce", C.byref(fa), C.byref(fy) if fy else None, C.byref(fm) if fm else None, _ptr(mean),
                          _ptr(invstd), _ptr(scale), _ptr(shift), 1 if relu else 0, C.byref(fz) if fz else None,
                          _ptr(partials), max_parts, C.byref(np_), _ptr(relu_bits),
                          keep=(fa, fy, fm, fz, np_, da, y, mask_src, dz_out, mean, invstd, scale, shift, partials,
                                relu_bits))
        return run, self._dry_parts(da, max_parts)

    def bn_bwd_finalize(self, partials, nparts, c, count, gamma, invstd, dgamma, dbeta, coef, workspace=None):
        return self._plain("sfk_bn_bwd_finalize", _ptr(partials), nparts, c, count, _ptr(gamma), _ptr(invstd),
                           _ptr(dgamma), _ptr(dbeta), _ptr(coef), _ptr(workspace),
                           keep=(partials, gamma, invstd, dgamma, dbeta, coef, workspace))

    def bn_bwd_apply(self, da: FMap, y: FMap, mask_src: Optional[FMap], mean, invstd, scale, shift, relu: bool, coef,
                     dy: FMap):
        fa, fy, fo = _c_fmap(da), _c_fmap(y), _c_fmap(dy)
        fm = _c_fmap(mask_src) if mask_src is not None else None
        return self._plain("sfk_bn_bwd_apply", C.byref(fa), C.byref(fy), C.byref(fm) if fm else None, _ptr(mean),
                           _ptr(invstd), _ptr(scale), _ptr(shift), 1 if relu else 0, _ptr(coef), C.byref(fo),
                           keep=(fa, fy, fo, fm, da, y, dy, mask_src, mean, invstd, scale, shift, coef))

    # -- the bottleneck tail (conv_c -> norm_c without the conv output in HBM)
    def bn_tail_fwd(self, gram, a_sums, a_nparts, count, g, c, w, cout, gamma, beta, eps, momentum, running_mean, running_var, nbt,
                    mean, invstd, scale, shift, t, wd=None):
        """gram [c][c]; a_sums: the partial column sums bn_apply left for `a` (a_nparts rows), folded into g [c] (kept for the
        backward); count = pixels.  wd: optional [c][cout] filter (A W)^T of the backward's first data-gradient pass"""
        ts = (gram, a_sums, g, w, gamma, beta, running_mean, running_var, nbt, mean, invstd, scale, shift, t, wd)
        return self._plain("sfk_bn_tail_fwd", _ptr(gram), _ptr(a_sums), a_nparts, count, _ptr(g), c, _ptr(w), _DT[w.dtype], cout,
                           _ptr(gamma), _ptr(beta), eps, momentum, _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(mean),
                           _ptr(invstd), _ptr(scale), _ptr(shift), _ptr(t), _ptr(wd), keep=ts)

    def bn_tail_bwd(self, r, dz_partials, nparts, g, count, t, c, w, cout, gamma, mean, invstd, dgamma, dbeta, dw, m,
                    bias, coef):
        """g [c], count: what bn_tail_fwd folded / was given.  m: [c][c] filter (compute precision) of the second
        data-gradient pass, W^T diag(B) W (include/sfk.h)"""
        ts = (r, dz_partials, g, t, w, gamma, mean, invstd, dgamma, dbeta, dw, m, bias, coef)
        return self._plain("sfk_bn_tail_bwd", _ptr(r), _ptr(dz_partials), nparts, _ptr(g), count, _ptr(t), c, _ptr(w),
                           _DT[w.dtype], cout, _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(dgamma), _ptr(dbeta), _ptr(dw),
                           _ptr(m), _ptr(bias), _ptr(coef), keep=ts)

    def conv_pw_dual_supported(self, x1: FMap, x2: FMap, y: FMap) -> bool:
        f1, f2, fy = _c_fmap(x1), _c_fmap(x2), _c_fmap(y)
        return bool(load().sfk_conv_pw_dual_supported(C.byref(f1), C.byref(f2), C.byref(fy)))

    def conv_pw_dual(self, x1: FMap, w1, x2: FMap, w2, bias, y: FMap):
        """y = x1 w1^T + x2 w2^T + bias in one pass (both data-gradient passes of a narrow block tail: include/sfk.h)"""
        f1, f2, fy = _c_fmap(x1), _c_fmap(x2), _c_fmap(y)
        return self._plain("sfk_conv_pw_dual", C.byref(f1), _ptr(w1), C.byref(f2), _ptr(w2), _ptr(bias), C.byref(fy),
                           keep=(f1, f2, fy, x1, x2, y, w1, w2, bias))

    # -- pooling / head / loss
    def maxpool_fwd(self, x: FMap, y: FMap, argmax, k, s, p):
        fx, fy = _c_fmap(x), _c_fmap(y)
        return self._plain("sfk_maxpool_fwd", C.byref(fx), C.byref(fy), _ptr(argmax), k, s, p, keep=(fx, fy, x, y, argmax))

    def maxpool_bwd(self, dy: FMap, argmax, dx: FMap, k, s, p):
        fy, fx = _c_fmap(dy), _c_fmap(dx)
        return self._plain("sfk_maxpool_bwd", C.byref(fy), _ptr(argmax), C.byref(fx), k, s, p, keep=(fx, fy, dx, dy, argmax))

    # -- the stem's BatchNorm -> ReLU -> MaxPool without the activation map (include/sfk.h sfk_bn_maxpool_*)
    @staticmethod
    def bn_maxpool_supported(k, s, p) -> bool:
        return (k, s, p) == (3, 2, 1)

    def bn_maxpool_fwd(self, y: FMap, scale, shift, out: FMap, argmax, k, s, p):
        fy, fo = _c_fmap(y), _c_fmap(out)
        return self._plain("sfk_bn_maxpool_fwd", C.byref(fy), _ptr(scale), _ptr(shift), C.byref(fo), _ptr(argmax), k, s, p,
                           keep=(fy, fo, y, out, scale, shift, argmax))

    def bn_maxpool_bwd_reduce(self, d_out: FMap, argmax, y: FMap, mean, invstd, scale, shift, partials, max_parts):
        """returns (run, nparts)"""
        fd, fy = _c_fmap(d_out), _c_fmap(y)
        np_ = C.c_int32(0)
        run = self._plain("sfk_bn_maxpool_bwd_reduce", C.byref(fd), _ptr(argmax), C.byref(fy), _ptr(mean), _ptr(invstd),
                          _ptr(scale), _ptr(shift), _ptr(partials), max_parts, C.byref(np_),
                          keep=(fd, fy, np_, d_out, y, argmax, mean, invstd, scale, shift, partials))
        return run, self._dry_parts(y, max_parts)

    def bn_maxpool_bwd_apply(self, d_out: FMap, argmax, y: FMap, mean, invstd, scale, shift, coef, dy: FMap):
        fd, fy, fo = _c_fmap(d_out), _c_fmap(y), _c_fmap(dy)
        return self._plain("sfk_bn_maxpool_bwd_apply", C.byref(fd), _ptr(argmax), C.byref(fy), _ptr(mean), _ptr(invstd),
                           _ptr(scale), _ptr(shift), _ptr(coef), C.byref(fo),
                           keep=(fd, fy, fo, d_out, y, dy, argmax, mean, invstd, scale, shift, coef))

    def head_pool_fwd(self, x: FMap, k, rate, seed, feat, feat_ld, f_off):
        fx = _c_fmap(x)
        return self._plain("sfk_head_pool_fwd", C.byref(fx), k[0], k[1], k[2], rate, _ptr(seed), _ptr(feat), feat_ld,
                           f_off, keep=(fx, x, seed, feat))

    def head_pool_bwd(self, dfeat, feat_ld, f_off, k, rate, seed, dx: FMap):
        fx = _c_fmap(dx)
        return self._plain("sfk_head_pool_bwd", _ptr(dfeat), feat_ld, f_off, k[0], k[1], k[2], rate, _ptr(seed),
                           C.byref(fx), keep=(fx, dx, seed, dfeat))

    def head_dropout_mask(self, n, c, f_off, positions, rate, seed, mask):
        return self._plain("sfk_head_dropout_mask", n, c, f_off, positions, rate, _ptr(seed), _ptr(mask), keep=(seed, mask))

    def fc_fwd(self, feat, w, b, logits, n, f, k):
        return self._plain("sfk_fc_fwd", _ptr(feat), _ptr(w), _ptr(b), _ptr(logits), n, f, k, keep=(feat, w, b, logits))

    def fc_bwd(self, dlogits, feat, w, dfeat, dw, db, n, f, k):
        return self._plain("sfk_fc_bwd", _ptr(dlogits), _ptr(feat), _ptr(w), _ptr(dfeat), _ptr(dw), _ptr(db), n, f, k,
                           keep=(dlogits, feat, w, dfeat, dw, db))

    def softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct):
        return self._plain("sfk_softmax_ce", _ptr(logits), _ptr(labels), n, k, gscale, _ptr(dlogits), _ptr(loss_out),
                           _ptr(loss_sum), _ptr(correct), keep=(logits, labels, dlogits, loss_out, loss_sum, correct))

    def softmax_ce_mix(self, logits, labels, rows, smoothing, n, k, gscale, dlogits, loss_out, loss_sum, correct):
        """sfk_softmax_ce_mix (include/sfk_mix.h): softmax_ce with the soft target of the mix table ``rows`` ((n, 8) float32
        on the device, or None: every row identity) and the label-smoothing mass ``smoothing`` in [0, 1)"""
        assert rows is None or (rows.dtype == torch.float32 and rows.is_contiguous() and tuple(rows.shape) == (n, MIX_ROW_FLOATS))
        return self._plain("sfk_softmax_ce_mix", _ptr(logits), _ptr(labels), _ptr(rows), smoothing, n, k, gscale,
                           _ptr(dlogits), _ptr(loss_out), _ptr(loss_sum), _ptr(correct),
                           keep=(logits, labels, rows, dlogits, loss_out, loss_sum, correct))

    # -- optimiser / misc
    def adam(self, p, g, m, v, count, lr, b1, b2, eps, gscale, step, shadow=None):
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        return self._plain("sfk_adam", _ptr(p), _ptr(g), _ptr(m), _ptr(v), count, lr, b1, b2, eps, gscale, _ptr(step),
                           _ptr(shadow), sd, keep=(p, g, m, v, step, shadow))

    def sgd(self, p, g, buf, count, lr, momentum, dampening, nesterov, gscale, step, shadow=None):
        """sfk_sgd (include/sfk_v2.h): torch.optim.SGD without weight decay; step[0] is incremented by the launch"""
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        return self._plain("sfk_sgd", _ptr(p), _ptr(g), _ptr(buf), count, lr, momentum, dampening, 1 if nesterov else 0,
                           gscale, _ptr(step), _ptr(shadow), sd, keep=(p, g, buf, step, shadow))

    @staticmethod
    def _optim_hp(lr_table, weight_decay, decay_mode, decay_count, clip_coef):
        assert lr_table.dtype == torch.float32 and lr_table.is_contiguous() and lr_table.dim() == 1
        assert clip_coef is None or clip_coef.dtype == torch.float32
        d = new_optim_hp()
        d.decay_mode = DECAY_MODES[decay_mode] if isinstance(decay_mode, str) else int(decay_mode)
        d.lr_table, d.lr_len, d.decay_count = lr_table.data_ptr(), lr_table.numel(), int(decay_count)
        d.clip_coef, d.weight_decay = _ptr(clip_coef), float(weight_decay)
        return d

    def adam_hp(self, p, g, m, v, count, lr_table, b1, b2, eps, gscale, step, shadow=None, weight_decay: float = 0.0,
                decay_mode="none", decay_count: int = 0, clip_coef=None):
        """sfk_adam_hp (include/sfk_optim.h): sfk_adam with the rate of step s read from lr_table[min(s, len) - 1] on the
        device, weight decay ('none' | 'l2' | 'decoupled') over elements [0, decay_count) and an optional clipping
        coefficient (device float[1])"""
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        d = self._optim_hp(lr_table, weight_decay, decay_mode, decay_count, clip_coef)
        return self._plain("sfk_adam_hp", _ptr(p), _ptr(g), _ptr(m), _ptr(v), count, C.byref(d), b1, b2, eps, gscale,
                           _ptr(step), _ptr(shadow), sd, keep=(d, p, g, m, v, step, shadow, lr_table, clip_coef))

    def sgd_hp(self, p, g, buf, count, lr_table, momentum, dampening, nesterov, gscale, step, shadow=None,
               weight_decay: float = 0.0, decay_mode="none", decay_count: int = 0, clip_coef=None):
        """sfk_sgd_hp (include/sfk_optim.h): sfk_sgd with the device rate table, L2 weight decay and clipping"""
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        d = self._optim_hp(lr_table, weight_decay, decay_mode, decay_count, clip_coef)
        return self._plain("sfk_sgd_hp", _ptr(p), _ptr(g), _ptr(buf), count, C.byref(d), momentum, dampening,
                           1 if nesterov else 0, gscale, _ptr(step), _ptr(shadow), sd,
                           keep=(d, p, g, buf, step, shadow, lr_table, clip_coef))

    def grad_norm_parts(self, count: int) -> int:
        """rows of float64 partial sums sfk_grad_norm needs for `count` gradients (a function of count alone)"""
        r = int(self.lib.sfk_grad_norm_parts(count))
        if r < 0:
            _check(r, "sfk_grad_norm_parts")
        return r

    def grad_norm(self, g, count, gscale, max_norm, partials, out):
        """sfk_grad_norm (include/sfk_optim.h): out[0] = ||g * gscale||_2, out[1] = min(1, max_norm / (out[0] + 1e-6));
        partials: float64[grad_norm_parts(count)], out: float32[2]"""
        assert partials.dtype == torch.float64 and partials.numel() >= self.grad_norm_parts(count)
        assert out.dtype == torch.float32 and out.numel() >= 2
        return self._plain("sfk_grad_norm", _ptr(g), count, gscale, max_norm, _ptr(partials), _ptr(out),
                           keep=(g, partials, out))

    def group_table(self, segments, weight_decays, count: int, device) -> GroupTable:
        """segments: sorted, disjoint (begin, end, group, decay) over [0, count); weight_decays: one per group (already
        wd * wd_mult).  Validates on the host (sfk_groups_prepare), fills tile0 and uploads the table once."""
        segments = [tuple(int(x) for x in s) for s in segments]
        n, ng = len(segments), len(weight_decays)
        host = (_GroupSeg * max(n, 1))()
        for k, (b, e, grp, dec) in enumerate(segments):
            host[k] = _GroupSeg(b, e, 0, grp, 1 if dec else 0)
        if n > GROUPS_MAX_SEGS:
            raise SfkError(f"sfk_groups_prepare: {n} segments, the cap is {GROUPS_MAX_SEGS}")
        tiles = int(self.lib.sfk_groups_prepare(C.addressof(host), n, count, ng))
        if tiles < 0:
            _check(tiles, "sfk_groups_prepare")
        raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8)[:n * C.sizeof(_GroupSeg)]
        dev = raw.to(device) if n else None
        wds = torch.tensor([float(w) for w in weight_decays], dtype=torch.float32).to(device)
        return GroupTable(segments, host, dev, wds, ng, count)

    @staticmethod
    def _groups_hp(table: GroupTable, lr_rows, decay_mode, clip_coef):
        assert lr_rows.dtype == torch.float32 and lr_rows.is_contiguous() and lr_rows.dim() == 2
        assert lr_rows.shape[0] == table.ngroups
        assert clip_coef is None or clip_coef.dtype == torch.float32
        d = _GroupsHp()
        d.struct_size = C.sizeof(_GroupsHp)
        d.decay_mode = DECAY_MODES[decay_mode] if isinstance(decay_mode, str) else int(decay_mode)
        d.segs, d.segs_host = _ptr(table.dev), (C.addressof(table.host) if table.nsegs else None)
        d.nsegs, d.ngroups = table.nsegs, table.ngroups
        d.lr_rows, d.lr_len = lr_rows.data_ptr(), lr_rows.shape[1]
        d.weight_decay, d.clip_coef = table.wds.data_ptr(), _ptr(clip_coef)
        return d

    def adam_groups(self, p, g, m, v, count, table: GroupTable, lr_rows, b1, b2, eps, gscale, step, shadow=None,
                    decay_mode="none", clip_coef=None):
        """sfk_adam_groups (include/sfk_groups.h): per segment [b, e) of group j the bits of adam_hp on that slice with
        lr_table = lr_rows[j], weight_decay = table's j-th, decay_count = decay ? e - b : 0; uncovered elements are frozen"""
        assert table.count == count
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        d = self._groups_hp(table, lr_rows, decay_mode, clip_coef)
        return self._plain("sfk_adam_groups", _ptr(p), _ptr(g), _ptr(m), _ptr(v), count, C.byref(d), b1, b2, eps, gscale,
                           _ptr(step), _ptr(shadow), sd, keep=(d, table, p, g, m, v, step, shadow, lr_rows, clip_coef))

    def sgd_groups(self, p, g, buf, count, table: GroupTable, lr_rows, momentum, dampening, nesterov, gscale, step,
                   shadow=None, decay_mode="none", clip_coef=None):
        """sfk_sgd_groups (include/sfk_groups.h): sgd_hp per segment, as adam_groups"""
        assert table.count == count
        sd = _DT[shadow.dtype] if shadow is not None else SFK_F32
        d = self._groups_hp(table, lr_rows, decay_mode, clip_coef)
        return self._plain("sfk_sgd_groups", _ptr(p), _ptr(g), _ptr(buf), count, C.byref(d), momentum, dampening,
                           1 if nesterov else 0, gscale, _ptr(step), _ptr(shadow), sd,
                           keep=(d, table, p, g, buf, step, shadow, lr_rows, clip_coef))

    def grad_norm_groups(self, g, count, table: GroupTable, gscale, max_norm, partials, out):
        """sfk_grad_norm_groups (include/sfk_groups.h): grad_norm over the covered elements only, the bits of grad_norm on a
        copy of g with the uncovered elements zeroed"""
        assert table.count == count
        assert partials.dtype == torch.float64 and partials.numel() >= self.grad_norm_parts(count)
        assert out.dtype == torch.float32 and out.numel() >= 2
        return self._plain("sfk_grad_norm_groups", _ptr(g), count, _ptr(table.dev),
                           C.addressof(table.host) if table.nsegs else None, table.nsegs, gscale, max_norm, _ptr(partials),
                           _ptr(out), keep=(table, g, partials, out))

    @staticmethod
    def _roi_strided_src(d, src):
        """the strided source of sfk_roi_resize and sfk_roi_resize_warp: its assertion and those fields of d; (n, t, c)"""
        n, t, h, w, c = src.shape
        assert src.dtype == torch.uint8
        d.src = src.data_ptr()
        d.sn, d.st, d.sh, d.sw, d.sc = src.stride()
        d.n, d.t, d.h, d.w, d.c = n, t, h, w, c
        return n, t, c

    @staticmethod
    def _roi_pool_src(d, pool, index, fill, c0, c):
        """the pool source of sfk_roi_resize_pool and sfk_roi_resize_pool_warp: its assertions and those fields of d; (n, t, c)"""
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and pool.stride(3) == 1 and 0 <= c0 and 0 < c and c0 + c <= p
        assert index.dtype == torch.int32 and index.dim() == 2 and index.is_contiguous()
        n, t = index.shape
        d.pool, d.index = pool.data_ptr(), index.data_ptr()
        d.frame_stride, d.row_stride, d.pixel_pitch = pool.stride(0), pool.stride(1), pool.stride(2)
        d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.fill = f, h, w, c0, c, n, t, int(fill)
        return n, t, c

    @staticmethod
    def _roi_ragged_src(d, arena, offset, hw, fill, pitch, c0, c, max_hw):
        """the arena source of sfk_roi_resize_ragged and sfk_roi_resize_ragged_warp: its assertions and those fields of d
        (max_hw None: read from hw, which synchronises); (n, t, c)"""
        c = pitch - c0 if c is None else c
        assert arena.dtype == torch.uint8 and arena.dim() == 1 and arena.is_contiguous() and 0 <= c0 and 0 < c and c0 + c <= pitch
        assert offset.dtype == torch.int64 and offset.dim() == 2 and offset.is_contiguous()
        n, t = offset.shape
        assert hw.dtype == torch.int32 and hw.is_contiguous() and tuple(hw.shape) == (n, 2)
        if max_hw is None:
            max_hw = tuple(max(int(v), 1) for v in hw.max(0).values.tolist())
        d.arena, d.arena_bytes, d.offset, d.hw = arena.data_ptr(), arena.numel(), offset.data_ptr(), hw.data_ptr()
        d.pixel_pitch, d.c0, d.c, d.n, d.t, d.fill = int(pitch), c0, c, n, t, int(fill)
        d.max_h, d.max_w = int(max_hw[0]), int(max_hw[1])
        return n, t, c

    @staticmethod
    def _roi_dst(d, n, t, c, lut, box, out, antialias, c_off, crop=None, pad=0, warp=None):
        """what the six sfk_roi_resize* descriptors share: the assertions on lut, box, out and on warp (the three _warp
        descriptors) or crop (the other three), and those fields of d"""
        assert lut.dtype == torch.float32 and lut.numel() == 256 and lut.is_contiguous()
        assert box.dtype == torch.int32 and box.is_contiguous() and tuple(box.shape) == (n, 4)
        assert out.dim() == 5 and out.stride(4) == 1 and out.shape[0] == n and out.shape[1] == t and 0 <= c_off and c_off + c <= out.shape[2]
        if warp is not None:
            assert warp.dtype == torch.float32 and warp.is_contiguous() and tuple(warp.shape) == (n, WARP_ROW_FLOATS)
            assert warp.device == out.device
            d.warp = warp.data_ptr()
        else:
            assert crop is None or (crop.dtype == torch.int32 and crop.is_contiguous() and tuple(crop.shape) == (n, 2))
            d.crop, d.pad = _ptr(crop), int(pad)
        d.antialias, d.lut, d.box = 1 if antialias else 0, lut.data_ptr(), box.data_ptr()
        d.out_h, d.out_w = out.shape[3], out.shape[4]
        d.dst_dtype, d.dst, d.c_off = _DT[out.dtype], out.data_ptr(), c_off
        d.dn, d.dt, d.dc, d.dh = out.stride()[:4]
        return d

    def roi_resize(self, src, lut, box, out, antialias: bool, crop=None, pad: int = 0, c_off: int = 0):
        """sfk_roi_resize (include/sfk_v2.h): src (N,T,H,W,C) uint8, any byte strides (HWC or a permuted planar view);
        box (N,4) int32 (x1, y1, x2, y2); out (N,T,C',S,S') f32|bf16 with unit W stride, channels c_off .. c_off+C-1 written;
        crop (N,2) int32 (top, left) or None."""
        d = new_roi_desc()
        d = self._roi_dst(d, *self._roi_strided_src(d, src), lut, box, out, antialias, c_off, crop, pad)
        return self._plain("sfk_roi_resize", C.byref(d), keep=(d, src, lut, box, out, crop))

    def color_jitter_workspace_bytes(self, n: int, t: int, h: int, w: int) -> int:
        """bytes of fp32 scratch sfk_color_jitter needs for n clips of t frames of h x w (include/sfk_aug.h)"""
        r = int(self.lib.sfk_color_jitter_workspace_bytes(n, t, h, w))
        if r < 0:
            _check(r, "sfk_color_jitter_workspace_bytes")
        return r

    def color_jitter(self, clip, params, workspace, c_off: int = 0, bgr: bool = False, mean: float = 0.0, std: float = 1.0):
        """sfk_color_jitter (include/sfk_aug.h): clip (N,T,C,H,W) f32|bf16 with unit W stride, channels c_off .. c_off+2
        jittered IN PLACE; params (N,8) float32 = order[4], b, c, s, h on the device, read when the launch runs; workspace:
        float32, color_jitter_workspace_bytes(N, T, H, W) bytes; stored value s <-> image value s*std + mean."""
        assert clip.dim() == 5 and clip.stride(4) == 1 and 0 <= c_off and c_off + 3 <= clip.shape[2]
        n, t, _, h, w = clip.shape
        assert params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == (n, 8)
        assert workspace.dtype == torch.float32 and workspace.numel() * 4 >= self.color_jitter_workspace_bytes(n, t, h, w)
        d = new_jitter_desc()
        d.dtype, d.x, d.params, d.workspace = _DT[clip.dtype], clip.data_ptr(), params.data_ptr(), workspace.data_ptr()
        d.sn, d.st, d.sc, d.sh = clip.stride()[:4]
        d.n, d.t, d.h, d.w = n, t, h, w
        d.c_off, d.bgr, d.mean, d.std = c_off, 1 if bgr else 0, mean, std
        return self._plain("sfk_color_jitter", C.byref(d), keep=(d, clip, params, workspace))

    def clip_mix(self, clip, rows, c_off: int = 0, c: Optional[int] = None):
        """sfk_clip_mix (include/sfk_mix.h): clip (N,T,C,H,W) f32|bf16 with unit W stride, channels c_off .. c_off+c-1 (c None:
        all from c_off) of every clip mixed IN PLACE with its partner's; rows (N,8) float32 = partner, lam, y0, x0, y1, x1,
        weight, reserved on the device, read when the launch runs."""
        assert clip.dim() == 5 and clip.stride(4) == 1
        n, t, ch, h, w = clip.shape
        c = ch - c_off if c is None else c
        assert 0 <= c_off and 0 < c and c_off + c <= ch
        assert rows.dtype == torch.float32 and rows.is_contiguous() and tuple(rows.shape) == (n, MIX_ROW_FLOATS)
        d = new_mix_desc()
        d.dtype, d.x, d.rows = _DT[clip.dtype], clip.data_ptr(), rows.data_ptr()
        d.sn, d.st, d.sc, d.sh = clip.stride()[:4]
        d.n, d.t, d.c, d.h, d.w, d.c_off = n, t, c, h, w, c_off
        return self._plain("sfk_clip_mix", C.byref(d), keep=(d, clip, rows))

    def ema_table(self, pairs) -> EmaTable:
        """pairs: (src, dst) float32 contiguous tensors of equal size on one device, src the live tensor and dst its average
        (include/sfk_ema.h sfk_ema_tensor).  Validates, uploads the table once and keeps the tensors alive."""
        pairs = [(s, d) for s, d in pairs]
        if len(pairs) > EMA_MAX_TENSORS:
            raise SfkError(f"sfk_ema table: {len(pairs)} tensors, the cap is {EMA_MAX_TENSORS}")
        host = (_EmaTensor * max(len(pairs), 1))()
        for k, (s, d) in enumerate(pairs):
            for t in (s, d):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != pairs[0][0].device:
                    raise SfkError(f"sfk_ema table entry {k}: float32 contiguous tensors on one device")
            if s.numel() != d.numel() or s.numel() < 1 or s.numel() >= 2 ** 31 or s.data_ptr() == d.data_ptr():
                raise SfkError(f"sfk_ema table entry {k}: src and dst are two tensors of the same size ({s.numel()}, {d.numel()})")
            host[k] = _EmaTensor(s.data_ptr(), d.data_ptr(), s.numel(), 0)
        dev = None
        if pairs:
            raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8)[:len(pairs) * C.sizeof(_EmaTensor)]
            dev = raw.to(pairs[0][0].device)
        return EmaTable(pairs, dev)

    @staticmethod
    def _ema_desc(p, e, count, table, decay, warmup, step):
        assert p.dtype == torch.float32 and e.dtype == torch.float32 and p.is_contiguous() and e.is_contiguous()
        assert 0 < count <= p.numel() and count <= e.numel() and p.data_ptr() != e.data_ptr()
        assert step is None or (step.dtype == torch.int64 and step.numel() >= 1)
        d = new_ema_desc()
        d.p, d.e, d.count, d.warmup, d.decay, d.step = p.data_ptr(), e.data_ptr(), int(count), 1 if warmup else 0, float(decay), _ptr(step)
        if table is not None:
            d.table, d.ntensors = _ptr(table.dev), table.ntensors
        return d

    def ema_update(self, p, e, count, table: Optional[EmaTable], decay: float, warmup: bool, step):
        """sfk_ema_update (include/sfk_ema.h): step[0] += 1 = t, w = (float)(1 - (warmup ? min(decay, (1 + t) / (10 + t)) :
        decay)), then e = e + w * (p - e) over the first count elements of the arenas and over every table pair"""
        d = self._ema_desc(p, e, count, table, decay, warmup, step)
        return self._plain("sfk_ema_update", C.byref(d), keep=(d, p, e, table, step))

    def ema_swap(self, p, e, count, table: Optional[EmaTable]):
        """sfk_ema_swap (include/sfk_ema.h): the bits of p and e, and of every table pair, exchanged"""
        d = self._ema_desc(p, e, count, table, 0.0, False, None)
        return self._plain("sfk_ema_swap", C.byref(d), keep=(d, p, e, table))

    @staticmethod
    def _fill_pool_desc(d, pool, index, lut, fill, out, c0, c, nt=None):
        """what sfk_pool_desc, sfk_pool_crop_desc and sfk_pool_warp_desc share: the assertions on pool, index, lut and out, and
        those fields of d.  index None (sfk_pool_warp_desc only): pool is the stacked batch, already viewed as (N*T,H,W,P),
        and nt its (N, T)"""
        f, h, w, p = pool.shape
        c = p - c0 if c is None else c
        assert pool.dtype == torch.uint8 and pool.stride(3) == 1 and 0 <= c0 and 0 < c and c0 + c <= p
        if index is not None:
            assert index.dtype == torch.int32 and index.dim() == 2 and index.is_contiguous()
            nt = index.shape
        n, t = nt
        assert lut.dtype == torch.float32 and lut.numel() == 256 and lut.is_contiguous()
        assert out.is_contiguous() and tuple(out.shape) == (n, t, c, h, w), (tuple(out.shape), (n, t, c, h, w))
        d.out_dtype, d.pool, d.index, d.lut, d.out = _DT[out.dtype], pool.data_ptr(), _ptr(index), lut.data_ptr(), out.data_ptr()
        d.frame_stride, d.row_stride, d.pixel_pitch = pool.stride(0), pool.stride(1), pool.stride(2)
        d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.fill = f, h, w, c0, c, n, t, int(fill)
        return d

    def u8_pool_gather(self, pool, index, lut, fill: int, out, c0: int = 0, c: Optional[int] = None):
        """sfk_u8_pool_gather (include/sfk_pool.h): pool (F,H,W,P) uint8 with unit channel stride (the byte strides are the
        tensor's), index (N,T) int32 on the device, read when the launch runs; out (N,T,c,H,W) f32|bf16 contiguous =
        lut[pool[index[n,t], y, x, c0 + ch]], or lut[fill] everywhere in a slab whose index is outside [0, F)."""
        d = self._fill_pool_desc(new_pool_desc(), pool, index, lut, fill, out, c0, c)
        return self._plain("sfk_u8_pool_gather", C.byref(d), keep=(d, pool, index, lut, out))

    def u8_pool_gather_crop(self, pool, index, lut, fill: int, crop, pad: int, out, c0: int = 0, c: Optional[int] = None):
        """sfk_u8_pool_gather_crop (include/sfk_resident.h): ``u8_pool_gather`` with RandomCrop's shift -- crop (N,2) int32
        (top, left) on the device, read when the launch runs, or None (no shift); out[n,t,ch,y,x] is 0 where
        (y + top - pad, x + left - pad) lies outside the frame, else the gathered value (lut[fill] for a missing frame)."""
        d = self._fill_pool_desc(new_pool_crop_desc(), pool, index, lut, fill, out, c0, c)
        if crop is not None:
            assert crop.dtype == torch.int32 and tuple(crop.shape) == (d.n, 2) and crop.is_contiguous()
            assert crop.device == index.device
        d.crop, d.pad = (None if crop is None else crop.data_ptr()), int(pad)
        return self._plain("sfk_u8_pool_gather_crop", C.byref(d), keep=(d, pool, index, lut, crop, out))

    def u8_pool_gather_warp(self, pool, index, lut, fill: int, warp, out, c0: int = 0, c: Optional[int] = None):
        """sfk_u8_pool_gather_warp (include/sfk_warp.h): ``u8_pool_gather_crop`` sampling through a matrix per clip -- warp
        (N,6) float32 (a, b, c, d, e, f) on the device, read when the launch runs: out[n,t,ch,y,x] is the bilinear sample of the
        normalised frame at (a x + b y + c, d x + e y + f), zeros outside the frame (lut[fill] for a missing frame).  index
        (N,T) int32, or None: pool is then the stacked batch (N,T,H,W,P) itself and clip n, time t reads frame n*T + t."""
        nt = None
        if index is None:
            assert pool.dim() == 5 and pool.is_contiguous(), "index=None: pool is the stacked (N,T,H,W,P) batch"
            nt = int(pool.shape[0]), int(pool.shape[1])
            pool = pool.view((nt[0] * nt[1],) + tuple(pool.shape[2:]))
        d = self._fill_pool_desc(new_pool_warp_desc(), pool, index, lut, fill, out, c0, c, nt)
        assert warp.dtype == torch.float32 and tuple(warp.shape) == (d.n, WARP_ROW_FLOATS) and warp.is_contiguous()
        assert warp.device == out.device
        d.warp = warp.data_ptr()
        return self._plain("sfk_u8_pool_gather_warp", C.byref(d), keep=(d, pool, index, lut, warp, out))

    def warp_fallback_tiles(self, h: int, w: int, pixel_pitch: int, c: int, row) -> int:
        """sfk_warp_fallback_tiles (include/sfk_warp.h), host only: how many output tiles of an h x w frame take their taps
        from global memory under the matrix row (6 floats) -- the staged box would not fit the launch's LDS"""
        m = (C.c_float * WARP_ROW_FLOATS)(*[float(v) for v in row])
        r = int(self.lib.sfk_warp_fallback_tiles(int(h), int(w), int(pixel_pitch), int(c), m))
        if r < 0:
            _check(r, "sfk_warp_fallback_tiles")
        return r

    def roi_resize_pool(self, pool, index, lut, fill: int, box, out, antialias: bool, crop=None, pad: int = 0, c0: int = 0,
                        c: Optional[int] = None, c_off: int = 0):
        """sfk_roi_resize_pool (include/sfk_roi_pool.h): ``roi_resize`` whose clip (n, t) is frame index[n, t] of pool
        (F,H,W,P) uint8 with unit channel stride, channels c0 .. c0+c-1 -- or the constant image of byte fill when the index
        is outside [0, F); index (N,T) int32, box (N,4) int32 and crop (N,2) int32 | None on the device, read when the launch
        runs; out (N,T,C',S,S') f32|bf16 with unit W stride, channels c_off .. c_off+c-1 written."""
        d = new_roi_pool_desc()
        d = self._roi_dst(d, *self._roi_pool_src(d, pool, index, fill, c0, c), lut, box, out, antialias, c_off, crop, pad)
        return self._plain("sfk_roi_resize_pool", C.byref(d), keep=(d, pool, index, lut, box, out, crop))

    def roi_resize_ragged(self, arena, offset, hw, lut, fill: int, box, out, antialias: bool, crop=None, pad: int = 0,
                          pitch: int = 7, c0: int = 0, c: Optional[int] = None, c_off: int = 0, max_hw=None):
        """sfk_roi_resize_ragged (include/sfk_roi_ragged.h): ``roi_resize`` whose clip (n, t) is the hw[n] = (h_n, w_n) pixels
        of ``pitch`` packed bytes at arena[offset[n, t]:], channels c0 .. c0+c-1 -- or the constant image of byte fill when
        that frame does not lie in the arena; arena 1-D uint8, 4-byte aligned, a multiple of 4 bytes; offset (N,T) int64, hw
        (N,2) int32, box (N,4) int32 in the rectangle's coordinates and crop (N,2) int32 | None on the device, read when the
        launch runs; max_hw = (max_h, max_w) bounds every hw row and sizes the tile (None: read from hw, which
        synchronises); out (N,T,C',S,S') f32|bf16 with unit W stride, channels c_off .. c_off+c-1 written."""
        d = new_roi_ragged_desc()
        ntc = self._roi_ragged_src(d, arena, offset, hw, fill, pitch, c0, c, max_hw)
        d = self._roi_dst(d, *ntc, lut, box, out, antialias, c_off, crop, pad)
        return self._plain("sfk_roi_resize_ragged", C.byref(d), keep=(d, arena, offset, hw, lut, box, out, crop))

    def roi_resize_warp(self, src, lut, box, warp, out, antialias: bool, c_off: int = 0):
        """sfk_roi_resize_warp (include/sfk_roi_warp.h): ``roi_resize`` sampled through a matrix per clip -- warp (N,6) float32
        (a, b, c, d, e, f) on the device, read when the launch runs: out[n,t,ch,y,x] is the resize's own interpolant at the
        position (a x + b y + c, d x + e y + f) of the resized image, zero outside it."""
        d = new_roi_warp_desc()
        d = self._roi_dst(d, *self._roi_strided_src(d, src), lut, box, out, antialias, c_off, warp=warp)
        return self._plain("sfk_roi_resize_warp", C.byref(d), keep=(d, src, lut, box, warp, out))

    def roi_resize_pool_warp(self, pool, index, lut, fill: int, box, warp, out, antialias: bool, c0: int = 0,
                             c: Optional[int] = None, c_off: int = 0):
        """sfk_roi_resize_pool_warp (include/sfk_roi_warp.h): ``roi_resize_pool`` sampled through warp (N,6) float32 as
        ``roi_resize_warp`` samples; a frame whose index is outside [0, F) is the constant image of byte fill."""
        d = new_roi_pool_warp_desc()
        d = self._roi_dst(d, *self._roi_pool_src(d, pool, index, fill, c0, c), lut, box, out, antialias, c_off, warp=warp)
        return self._plain("sfk_roi_resize_pool_warp", C.byref(d), keep=(d, pool, index, lut, box, warp, out))

    def roi_resize_ragged_warp(self, arena, offset, hw, lut, fill: int, box, warp, out, antialias: bool, pitch: int = 7,
                               c0: int = 0, c: Optional[int] = None, c_off: int = 0, max_hw=None):
        """sfk_roi_resize_ragged_warp (include/sfk_roi_warp.h): ``roi_resize_ragged`` sampled through warp (N,6) float32 as
        ``roi_resize_warp`` samples; a frame that does not lie in the arena whole is the constant image of byte fill."""
        d = new_roi_ragged_warp_desc()
        ntc = self._roi_ragged_src(d, arena, offset, hw, fill, pitch, c0, c, max_hw)
        d = self._roi_dst(d, *ntc, lut, box, out, antialias, c_off, warp=warp)
        return self._plain("sfk_roi_resize_ragged_warp", C.byref(d), keep=(d, arena, offset, hw, lut, box, warp, out))

    def u8_pad_resize_cubic(self, src, offset, hw, out, size: int, max_side: int, fill: int):
        """sfk_u8_pad_resize_cubic (include/sfk_resize.h): src 1-D uint8, the frames' HWC bytes; offset (F,) int64 and hw (F, 2)
        int32 on the device, read when the launch runs; out (F, size, size, c) uint8 -- or (N, T, size, size, c), F = N*T --
        whose frames are contiguous and evenly spaced: out_frame_stride is the tensor's.  A frame with a non-positive or
        oversized (h, w), or a span outside src, becomes bytes of fill."""
        assert src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()
        assert offset.dtype == torch.int64 and offset.dim() == 1 and offset.is_contiguous()
        f = offset.shape[0]
        assert hw.dtype == torch.int32 and tuple(hw.shape) == (f, 2) and hw.is_contiguous()
        assert out.dtype == torch.uint8 and out.dim() in (4, 5)
        c = out.shape[-1]
        assert tuple(out.shape[-3:]) == (size, size, c) and tuple(out.stride()[-3:]) == (size * c, c, 1), tuple(out.stride())
        if out.dim() == 5:
            assert out.shape[0] * out.shape[1] == f and (out.shape[0] == 1 or out.stride(0) == out.shape[1] * out.stride(1))
        else:
            assert out.shape[0] == f
        d = new_resize_desc()
        d.src, d.src_bytes, d.offset, d.hw, d.out = src.data_ptr(), src.numel(), offset.data_ptr(), hw.data_ptr(), out.data_ptr()
        d.frames, d.c, d.size, d.max_side, d.fill = f, c, int(size), int(max_side), int(fill)
        d.out_frame_stride = out.stride(-4)
        return self._plain("sfk_u8_pad_resize_cubic", C.byref(d), keep=(d, src, offset, hw, out))

    def filter_transpose(self, src, dst, cout, wtaps, cin):
        return self._plain("sfk_filter_transpose", _ptr(src), _DT[src.dtype], _ptr(dst), _DT[dst.dtype], cout, wtaps,
                           cin, keep=(src, dst))

    def cast(self, src, dst, count):
        return self._plain("sfk_cast", _ptr(src), _DT[src.dtype], _ptr(dst), _DT[dst.dtype], count, keep=(src, dst))

    def filter_refresh(self, master, s, st, layers):
        """layers: [(arena offset, cout, wtaps, cin, transpose)], one launch for all of them (sfk_filter_refresh)."""
        import numpy as np
        ent = np.zeros(len(layers), dtype=np.dtype([("off", "<i8"), ("cout", "<i4"), ("wtaps", "<i4"), ("cin", "<i4"),
                                                    ("first_block", "<i4"), ("transpose", "<i4"), ("reserved", "<i4")]))
        fb = 0
        for i, (off, cout, wtaps, cin, tr) in enumerate(layers):
            ent[i] = (off, cout, wtaps, cin, fb, 1 if tr else 0, 0)
            fb += wtaps * ((cout + 31) // 32) * ((cin + 31) // 32)
        table = torch.from_numpy(ent.view(np.uint8).copy()).to(master.device)
        ref = st if st is not None else s
        return self._plain("sfk_filter_refresh", _ptr(master), _ptr(s), _ptr(st), _DT[ref.dtype], _ptr(table),
                           len(layers), fb, keep=(master, s, st, table))

    def u8_normalize_crop(self, src_u8, lut, crop, pad: int, out):
        """src_u8 (N,T,H,W,C) uint8 -> out (N,T,C,H,W) f32|bf16 = lut[byte], shifted by the per-clip crop (or None)"""
        n, t, h, w, c = src_u8.shape
        assert src_u8.dtype == torch.uint8 and src_u8.is_contiguous() and out.is_contiguous()
        assert tuple(out.shape) == (n, t, c, h, w)
        return self._plain("sfk_u8_normalize_crop", _ptr(src_u8), _ptr(lut), _ptr(crop), pad, _ptr(out), _DT[out.dtype],
                           n, t, c, h, w, keep=(src_u8, lut, crop, out))

    def eval_aggregate(self, logits, labels, seg_off, nvideos: int, softmax: bool, ps_out, pred, correct):
        return self._plain("sfk_eval_aggregate", _ptr(logits), _ptr(labels), _ptr(seg_off), nvideos, logits.shape[1],
                           1 if softmax else 0, _ptr(ps_out), _ptr(pred), _ptr(correct),
                           keep=(logits, labels, seg_off, ps_out, pred, correct))

    def sparse_fusion_fwd(self, x, w, b, y, n, p, c):
        return self._plain("sfk_sparse_fusion_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y), n, p, c, keep=(x, w, b, y))

    def sparse_fusion_bwd(self, x, dy, dw, db, n, p, c):
        return self._plain("sfk_sparse_fusion_bwd", _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), n, p, c, keep=(x, dy, dw, db))

    def fill_zero(self, t: torch.Tensor):
        return self._plain("sfk_fill_zero", t.data_ptr(), t.numel() * t.element_size(), keep=(t,))
