"""TEST INFRASTRUCTURE: the contract of include/sfk.h (as tests/emu_backend.py states it) restated in float64, on whatever
device its arguments live on, plus the one tolerance policy every launch-audit comparison uses.

Every GEMM-like restatement returns (value, a) with a = the same sum over |terms| (the GEMM on absolute values): the
element-wise bound is built from it.  Convolutions, data and filter gradients are sums over taps of gathered inputs times
per-tap matrices (float64 matmuls, no F.conv3d), so the restatement shares no code path with the kernels or with torch's
convolution."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

F64 = torch.float64

# ----------------------------------------------------------------------------- tolerance policy
EPS32 = 2.0 ** -24
# aggregate ||y - r|| / ||r|| per output kind: a bf16 map carries its rounding (<= 2^-9 relative per element); fp32 results of
# long sums (filter gradients, BatchNorm partial sums, coefficients) carry fp32 accumulation only
# long sums (filter gradients, BatchNorm partial sums, coefficients) carry fp32 accumulation only.  sum_f32_fused: the partial
# sums (sum dz, sum dz * x_hat) a data-gradient pass leaves from its epilogue (sfk_bn_bwd_fuse): measured at 1.1e-5 .. 1.5e-5
# at the production geometries (the stand-alone sfk_bn_bwd_reduce: < 1e-7) -- these column sums cancel to ~sqrt(pixels) of
# their terms, so the fp32 accumulation of the epilogue's long per-thread runs shows; 2^-9 below the bf16 rounding of dz itself
AGG_BOUND = {"map_bf16": 2.0 ** -9, "map_f32": 1e-5, "sum_f32": 1e-5, "sum_f32_fused": 4e-5}


def ulp_out(r: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """one unit in the last place of r in `dtype` (bf16: 8 significant bits, fp32: 24)"""
    p = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    _, e = torch.frexp(r.double())
    u = torch.ldexp(torch.ones_like(r, dtype=F64), (e - 1 - p))
    tiny = {torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}[dtype]
    return u.clamp_min(tiny)


def elem_bound(r: torch.Tensor, a: torch.Tensor, k: float, dtype: torch.dtype) -> torch.Tensor:
    """|y - r| <= ulp_out(r) + 2^-24 (16 + 2 sqrt(K)) a"""
    return ulp_out(r, dtype) + EPS32 * (16.0 + 2.0 * math.sqrt(max(float(k), 1.0))) * a.double()


class Verdict:
    __slots__ = ("name", "kind", "worst", "agg", "agg_bound", "n", "ok", "where")

    def __init__(self, name, kind, worst, agg, agg_bound, n, where=None):
        self.name, self.kind, self.worst, self.agg, self.agg_bound, self.n = name, kind, worst, agg, agg_bound, n
        self.where = where
        self.ok = worst <= 1.0 and agg <= agg_bound

    def __repr__(self):
        w = f" at {self.where}" if self.where is not None and (self.worst > 1.0 or isinstance(self.where, str)) else ""
        return (f"{self.name}[{self.kind}] worst {self.worst:.3g}{w} agg {self.agg:.3g}/{self.agg_bound:.3g} "
                f"n {self.n} {'ok' if self.ok else 'FAIL'}")


def compare(name: str, y: torch.Tensor, r: torch.Tensor, a: torch.Tensor, k: float, dtype: torch.dtype, kind: str,
            alt: Optional[torch.Tensor] = None, alt_mask: Optional[torch.Tensor] = None) -> Verdict:
    """The tolerance policy.  y: the kernel's values, r: the float64 reference, a: its sum of |terms|, k: its reduction length,
    dtype: the output's storage type, kind: a key of AGG_BOUND.  alt / alt_mask: where the reference itself is ambiguous (a
    ReLU mask on a value within its own error of zero), y may match `alt` instead of `r`."""
    y, r = y.double().reshape(-1), r.double().reshape(-1)
    a = a.double().reshape(-1) if torch.is_tensor(a) else torch.full_like(r, float(a))
    if y.numel() == 0:
        return Verdict(name, kind, 0.0, 0.0, AGG_BOUND[kind], 0)
    bnd = elem_bound(r, a, k, dtype)
    err = (y - r).abs()
    if alt is not None:
        alt = alt.double().reshape(-1)
        am = alt_mask.reshape(-1)
        err_alt = (y - alt).abs()
        bnd_alt = elem_bound(alt, a, k, dtype)
        ratio = torch.where(am, torch.minimum(err / bnd, err_alt / bnd_alt), err / bnd)
        rr = torch.where(am & (err_alt / bnd_alt < err / bnd), alt, r)
    else:
        ratio, rr = err / bnd, r
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst_i = int(torch.argmax(ratio))
    worst = float(ratio[worst_i])
    den = float(rr.norm())
    num = float((y - rr).norm())
    agg = num / den if den > 0 else (0.0 if num == 0 else float("inf"))
    if not math.isfinite(agg):
        agg = float("inf")
    return Verdict(name, kind, worst, agg, AGG_BOUND[kind], r.numel(), where=worst_i)


SMALL_MAP = 2048               # elements below which a bf16 map's aggregate ratio says nothing (see elem_only)


def elem_only(kind: str, n: int) -> bool:
    """The aggregate bound of a bf16 map (2^-9) is the rms of a rounding error uniform in +- half an ulp -- 0.0016 to 0.0017
    for honest rounding -- and is met only once many elements average out: EmuBackend's correctly rounded 8-, 24- and
    80-element maps come out at 0.0020 to 0.0022.  Below SMALL_MAP elements such a map is therefore judged by its element
    bound alone, as a lone scalar is.  The ONE statement of that rule: bn_ref64.compare and launch_audit.replay use it."""
    return kind == "map_bf16" and n < SMALL_MAP


def judge(name, y, r, a, k, dtype, kind, alt=None, alt_mask=None) -> Verdict:
    """compare(), with a map that elem_only() names judged by its element bound alone (agg is still reported)"""
    v = compare(name, y, r, a, k, dtype, kind, alt=alt, alt_mask=alt_mask)
    if elem_only(kind, v.n):
        v.agg_bound = float("inf")
        v.ok = v.worst <= 1.0
    return v


def rounded(r: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return r.to(dtype).double()


# ----------------------------------------------------------------------------- gathers and GEMMs
def gather(X: torch.Tensor, rows: Sequence[int], gs: Sequence[int], d: Sequence[int]) -> torch.Tensor:
    """X (N,T,H,W,C) -> (N, rt, rh, rw, C) with element [n, r] = X[n, r*gs + d], zero outside X's extents"""
    pads, sl = [], []
    for r, g, dd, ext in zip(rows, gs, d, X.shape[1:4]):
        last = (r - 1) * g + dd
        lo, hi = max(0, -dd), max(0, last - (ext - 1))
        pads.append((lo, hi))
        sl.append(slice(dd + lo, dd + lo + (r - 1) * g + 1, g))
    if any(p != (0, 0) for p in pads):
        (t0, t1), (h0, h1), (w0, w1) = pads
        X = torch.nn.functional.pad(X, (0, 0, w0, w1, h0, h1, t0, t1))
    return X[:, sl[0], sl[1], sl[2]]


def conv(X: torch.Tensor, W: torch.Tensor, rows, gs, taps) -> Tuple[torch.Tensor, torch.Tensor]:
    """sfk_conv_igemm's accumulator: acc[n, r, co] = sum_taps sum_ci X[n, r*gs + tap.d, ci] W[co, tap.widx, ci].
    X (N,T,H,W,Cin), W (Cout, wtaps, Cin) -> acc, a (N, rt, rh, rw, Cout) float64"""
    X, W = X.to(F64), W.to(F64)
    Xa, Wa = X.abs(), W.abs()
    acc = torch.zeros(X.shape[0], *rows, W.shape[0], dtype=F64, device=X.device)
    a = torch.zeros_like(acc)
    for dt, dh, dw, wi in taps:
        acc += gather(X, rows, gs, (dt, dh, dw)) @ W[:, wi, :].t()
        a += gather(Xa, rows, gs, (dt, dh, dw)) @ Wa[:, wi, :].t()
    return acc, a


def wgrad(X: torch.Tensor, dY: torch.Tensor, gs, taps, wtaps: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """sfk_conv_wgrad's sum: dw[co, widx, ci] = sum_rows dY[n, r, co] X[n, r*gs + tap.d, ci] (taps not listed stay 0)"""
    X, dY = X.to(F64), dY.to(F64)
    rows = tuple(dY.shape[1:4])
    D, Da = dY.reshape(-1, dY.shape[-1]), dY.abs().reshape(-1, dY.shape[-1])
    cin = X.shape[-1]
    dw = torch.zeros(dY.shape[-1], wtaps, cin, dtype=F64, device=X.device)
    a = torch.zeros_like(dw)
    for dt, dh, dwd, wi in taps:
        G = gather(X, rows, gs, (dt, dh, dwd)).reshape(-1, cin)
        dw[:, wi, :] += D.t() @ G
        a[:, wi, :] += Da.t() @ G.abs()
    return dw, a


def region(rows, os_, oo) -> Tuple[slice, slice, slice]:
    return tuple(slice(o, o + (r - 1) * s + 1, s) for o, s, r in zip(oo, os_, rows))


# ----------------------------------------------------------------------------- stems
def stem_taps(kt: int):
    """the stem conv (kt,7,7) stride (1,2,2) pad (kt//2,3,3) as an implicit-GEMM tap table over W (cout, kt*49, cin)"""
    return [(f - kt // 2, kh - 3, kw - 3, (f * 7 + kh) * 7 + kw) for f in range(kt) for kh in range(7) for kw in range(7)]


def stem_w(w: torch.Tensor, cout: int, cin: int, kt: int, kp: int) -> torch.Tensor:
    """stem layout [co][((f*cin+ci)*7+kh)*8+kw] -> (cout, kt*49, cin) float64"""
    v = w[: cout * kp].view(cout, kp)[:, : kt * cin * 56].to(F64).view(cout, kt, cin, 7, 8)[..., :7]
    return v.permute(0, 1, 3, 4, 2).reshape(cout, kt * 49, cin)


def stem_w_layout(g: torch.Tensor, cout: int, cin: int, kt: int) -> torch.Tensor:
    """(cout, kt*49, cin) -> (cout, kt*cin*56) in the stem layout (kw = 7 column zero)"""
    v = g.view(cout, kt, 7, 7, cin).permute(0, 1, 4, 2, 3)
    return torch.nn.functional.pad(v, (0, 1)).reshape(cout, kt * cin * 56)


def stem_x(src: torch.Tensor, t_index: Optional[torch.Tensor], dtype) -> torch.Tensor:
    """the clip (n, c, t, h, w), rounded to the compute precision as the kernels stage it, frames gathered -> (N,T,H,W,C)"""
    x = src.to(dtype).to(F64)
    if t_index is not None:
        x = x.index_select(2, t_index.long())
    return x.permute(0, 2, 3, 4, 1)


def stem2d_x(src: torch.Tensor, dtype) -> torch.Tensor:
    """frames-as-channels: (n, c, t, h, w) -> (N, 1, H, W, T*C), channel t*C + c"""
    x = src.to(dtype).to(F64)
    n, c, t, h, w = x.shape
    return x.permute(0, 3, 4, 2, 1).reshape(n, 1, h, w, t * c)


# ----------------------------------------------------------------------------- BatchNorm and the stem tail
def relu_bits_unpack(bits: torch.Tensor, pixels: int, c: int, vec: int) -> torch.Tensor:
    """byte [pixel][c / vec], bit i = channel group*vec + i -> bool (pixels, c)"""
    b = bits[: pixels * (c // vec)].to(torch.int32).reshape(pixels, c // vec, 1)
    sh = torch.arange(vec, dtype=torch.int32, device=bits.device)
    return ((b >> sh) & 1).reshape(pixels, c).bool()


def relu_bits_pack(m: torch.Tensor, vec: int) -> torch.Tensor:
    """bool (pixels, c) -> uint8 (pixels * c / vec)"""
    p, c = m.shape
    w = (1 << torch.arange(vec, dtype=torch.int32, device=m.device))
    return (m.reshape(p, c // vec, vec).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)


def bn_pre(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """v = y*scale + shift in float64 and the bound on how far an fp32 evaluation of it can be from v"""
    y, sc, sh = y.to(F64), scale.to(F64), shift.to(F64)
    v = y * sc + sh
    return v, 4 * EPS32 * ((y * sc).abs() + sh.abs())


def maxpool_fwd(a: torch.Tensor, k: int, s: int, p: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaxPool (1,k,k)/(1,s,s)/(0,p,p) of a (N,T,H,W,C): (out, argmax = kh*k + kw of the first maximum in scan order)"""
    n, t, h, w, c = a.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    best = torch.full((n, t, ho, wo, c), -math.inf, dtype=a.dtype, device=a.device)
    arg = torch.zeros((n, t, ho, wo, c), dtype=torch.uint8, device=a.device)
    for kh in range(k):
        for kw in range(k):
            hi = torch.arange(ho, device=a.device) * s - p + kh
            wi = torch.arange(wo, device=a.device) * s - p + kw
            ok = (((hi >= 0) & (hi < h)).view(1, 1, -1, 1, 1) & ((wi >= 0) & (wi < w)).view(1, 1, 1, -1, 1))
            v = gather(a, (t, ho, wo), (1, s, s), (0, kh - p, kw - p))
            take = ok & (v > best)
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.full_like(arg, kh * k + kw), arg)
    return best, arg


def maxpool_bwd(d_out: torch.Tensor, arg: torch.Tensor, h: int, w: int, k: int, s: int, p: int) -> torch.Tensor:
    """da (N,T,h,w,C) = sum over windows of [argmax == tap] d_out, float64 (scatter-add on a padded frame)"""
    n, t, ho, wo, c = d_out.shape
    hp, wp = max(h + 2 * p, (ho - 1) * s + k), max(w + 2 * p, (wo - 1) * s + k)
    da = torch.zeros(n, t, hp, wp, c, dtype=F64, device=d_out.device)
    g = d_out.to(F64)
    for kh in range(k):
        for kw in range(k):
            sel = (arg == kh * k + kw).to(F64)
            da[:, :, kh:kh + (ho - 1) * s + 1:s, kw:kw + (wo - 1) * s + 1:s] += g * sel
    return da[:, :, p:p + h, p:p + w]
