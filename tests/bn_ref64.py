"""TEST INFRASTRUCTURE: the band of kernels between the conv launches and the head -- sfk_bn_apply (all six forms, relu_bits,
out_sums), sfk_bn_bwd_apply, sfk_bn_finalize / sfk_bn_eval_coeffs / sfk_bn_bwd_finalize, sfk_maxpool_fwd / bwd and the block-tail
algebra sfk_bn_tail_fwd / bwd -- restated in float64 from the contract text of include/sfk.h, the case tables, and the checks
that run one case on a backend (HipBackend on the GPU, EmuBackend and its mutants on the CPU) and return the verdicts.

Every comparison goes through ref64.compare as it stands: |y - r| <= ulp(r) + 2^-24 (16 + 2 sqrt(K)) a, a = the reference's sum
over |terms|, K = the longest fp32 accumulation behind the value.  No tolerance is added.  Where a value is DERIVED from another
one that carries an error (invstd from var, scale from invstd, shift from mean * scale, the coefficients of the tail), `a` is
propagated through the derivative, and the derivation stands next to it (bn_derived, tail_bwd_ref).

A ReLU decision on a pre-activation v within an fp32 evaluation's own error of zero is ambiguous: there the output may match
the other branch (alt / alt_mask of ref64.compare) and the bitmap may hold either bit.  The share of such elements is computed
from the float64 reference alone and has to stay below AMB_CAP in every case."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

import ref64
from head_ref64 import ElemOnly, Exact, _stream, _sync, f32, failures, worst_of  # noqa: F401  (re-exported for the tests)
from ref64 import EPS32, F64, relu_bits_pack, relu_bits_unpack
from video_classification_amd._lib import BN_FOLD_ROWS, FMap

F32, BF16 = torch.float32, torch.bfloat16
SENT = -7.5                    # exactly representable in bf16 and fp32
BYTE_SENT = 0xA5
GUARD = 64                     # elements behind every buffer that no kernel may touch
AMB_CAP = 1e-3                 # share of ambiguous ReLU signs a case may excuse
EPS, MOMENTUM = 1e-5, 0.1
SPAN_U = 4                     # pixel rows a thread of the streaming kernels handles per span (csrc/bn.hip SFK_BN_U)
GRID_CAP = 65535               # blocks of the apply grids (csrc/bn.hip span_blocks)


SMALL_MAP = ref64.SMALL_MAP     # elements below which a bf16 map's aggregate ratio says nothing (ref64.elem_only)


def compare(name, y, r, a, k, dtype, kind, alt=None, alt_mask=None):
    """ref64.judge: ref64.compare, with a bf16 map that ref64.elem_only names (fewer than SMALL_MAP elements) judged by its
    element bound alone, as a lone scalar is"""
    return ref64.judge(name, y, r, a, k, dtype, kind, alt=alt, alt_mask=alt_mask)


def vec_of(dtype) -> int:
    return 8 if dtype == BF16 else 4


def kind_of(dtype) -> str:
    return "map_bf16" if dtype == BF16 else "map_f32"


def tag_of(dtype) -> str:
    return "bf16" if dtype == BF16 else "f32"


def rows_b(c: int, dtype) -> int:
    """pixel rows a 256-thread block of the streaming kernels covers at once (csrc/bn.hip ChanMap)"""
    return 256 // min(c // vec_of(dtype), 256)


def dims_of(px: int) -> Tuple[int, int, int, int]:
    """(n, t, h, w) with n t h w = px: small prime factors peeled off into n, t, h"""
    out = []
    for _ in range(3):
        f = next((q for q in (2, 3, 5, 7) if px % q == 0 and px > q), 1)
        out.append(f)
        px //= f
    return out[0], out[1], out[2], px


def _bits(t: torch.Tensor) -> torch.Tensor:
    v = {BF16: torch.int16, F32: torch.int32}.get(t.dtype)
    return t if v is None else t.view(v)


def _in_map(gen, dev, dtype, dims, c, ld, off) -> FMap:
    """an input map whose whole buffer -- padding columns and guard included -- holds random data"""
    px = dims[0] * dims[1] * dims[2] * dims[3]
    return FMap(torch.randn(px * ld + GUARD, generator=gen).to(dtype).to(dev), *dims, c, ld, off)


def _out_map(dev, dtype, dims, c, ld, off) -> FMap:
    px = dims[0] * dims[1] * dims[2] * dims[3]
    return FMap(torch.full((px * ld + GUARD,), SENT, dtype=dtype, device=dev), *dims, c, ld, off)


def _view(m: FMap, buf: torch.Tensor) -> torch.Tensor:
    return FMap(buf, m.n, m.t, m.h, m.w, m.c, m.ld, m.c_off).view5()


def _vecbuf(x: torch.Tensor, dev, dtype=F32) -> torch.Tensor:
    """x followed by GUARD sentinels"""
    out = torch.full((x.numel() + GUARD,), SENT, dtype=dtype, device=dev)
    out[: x.numel()] = x.reshape(-1).to(dtype)
    return out


def _sentbuf(n: int, dev, dtype=F32) -> torch.Tensor:
    return torch.full((n + GUARD,), SENT, dtype=dtype, device=dev)


def untouched(name: str, m: FMap, before: torch.Tensor) -> Exact:
    """every element of m's buffer outside the map's channel slice, the guard included, still holds what it held"""
    keep = torch.ones(m.buf.numel(), dtype=torch.bool, device=m.buf.device)
    keep[: m.pixels * m.ld].view(m.pixels, m.ld)[:, m.c_off:m.c_off + m.c] = False
    return Exact(name, torch.equal(_bits(m.buf)[keep], _bits(before)[keep]), f"{int(keep.sum())} elements outside the slice")


def same(name: str, t: torch.Tensor, before: torch.Tensor) -> Exact:
    return Exact(name, torch.equal(_bits(t), _bits(before)), f"{t.numel()} elements")


def guard_ok(name: str, bufs, n_used) -> Exact:
    """the elements past n_used[i] of bufs[i] still hold the sentinel"""
    ok = all(bool((b[n:].double() == (BYTE_SENT if b.dtype == torch.uint8 else SENT)).all()) for b, n in zip(bufs, n_used))
    return Exact(name, ok, f"{len(bufs)} buffers")


def amb_share(name: str, amb: Optional[torch.Tensor]) -> Exact:
    share = 0.0 if amb is None or amb.numel() == 0 else float(amb.double().mean())
    return Exact(f"ambiguous ReLU signs {name}", share < AMB_CAP, f"{share:.2g} of the elements (cap {AMB_CAP})")


# ----------------------------------------------------------------------------- sfk_bn_apply
def apply_ref(y, scale, shift, res=None, rs=None, rb=None):
    """v = y*scale + shift + (0 | res | res*rs + rb) in float64, a = the sum of |terms|, amb = |v| within what an fp32
    evaluation of it can be off by: at most five roundings (two products, three sums), each <= 2^-24 of a partial sum <= a,
    one more for a fused or reordered form"""
    yv, sc, sh = y.to(F64), scale.to(F64), shift.to(F64)
    v, a = yv * sc + sh, (yv * sc).abs() + sh.abs()
    if res is not None:
        r = res.to(F64)
        if rs is not None:
            v, a = v + r * rs.to(F64) + rb.to(F64), a + (r * rs.to(F64)).abs() + rb.to(F64).abs()
        else:
            v, a = v + r, a + r.abs()
    return v, a, v.abs() <= 6.0 * EPS32 * a


def _apply_px(c, dtype) -> List[int]:
    """1 pixel; fewer pixels than rows_b (where rows_b > 1); two whole spans plus 1, 2, 3 rows of the third: the first of
    these is 4 rows_b blocks + 1"""
    rb = rows_b(c, dtype)
    return [1] + ([rb - 1] if rb > 2 else []) + [SPAN_U * rb * 2 + (r - 1) * rb + 1 for r in (1, 2, 3)]


CMULS = (1, 10, 256, 288)      # channel groups: one group; 25 rows per block and 6 idle threads; one chunk; a partial second chunk


def _apply_cases():
    out = []
    for dtype in (BF16, F32):
        V = vec_of(dtype)
        for cm in CMULS:
            for res in (0, 1, 2):
                for relu in (False, True):
                    for px in _apply_px(cm * V, dtype):
                        out.append(dict(dtype=dtype, cm=cm, c=cm * V, px=px, res=res, relu=relu, alias=False, sums=None))
        out.append(dict(dtype=dtype, cm=10, c=10 * V, px=251, res=1, relu=True, alias=True, sums=None))
        out.append(dict(dtype=dtype, cm=288, c=288 * V, px=11, res=2, relu=False, alias=True, sums=None))
    return out


def _sums_cases():
    """max_parts 1 / 3 / the uncapped value; 7 spans + 1 pixel (on 3 blocks the third trip leaves the last block no row) and
    3001 pixels (the grid-stride loop runs several trips)"""
    out = []
    for dtype in (BF16, F32):
        V = vec_of(dtype)
        for cm in CMULS:
            for mp in (1, 3, 1024):
                for px in (SPAN_U * rows_b(cm * V, dtype) * 7 + 1, 3001):
                    out.append(dict(dtype=dtype, cm=cm, c=cm * V, px=px, res=0, relu=True, alias=False, sums=mp))
    return out


def case_name(case) -> str:
    s = f"{tag_of(case['dtype'])}-c{case['c']}-px{case['px']}"
    if "mask" in case:
        return s + f"-mask{case['mask']}{'-inplace' if case['inplace'] else ''}"
    s += f"-res{case['res']}{'-relu' if case['relu'] else ''}{'-alias' if case['alias'] else ''}"
    return s + (f"-parts{case['sums']}" if case["sums"] else "")


APPLY_CASES = _apply_cases()
SUMS_CASES = _sums_cases()
APPLY_GROUPS = [(d, cm) for d in (BF16, F32) for cm in CMULS]


def group_of(cases, dtype, cm):
    return [c for c in cases if c["dtype"] == dtype and c["cm"] == cm]


def _coef(gen, dev, c, kind):
    if kind == "scale":                         # in [0.5, 1.5]
        return (torch.rand(c, generator=gen) + 0.5).to(dev)
    return (0.3 * torch.randn(c, generator=gen)).to(dev)


def check_apply(be, dev, case, seed_no: int = 0) -> List:
    """one sfk_bn_apply launch: the output against float64, the bitmap against the reference sign, the column sums against
    the float64 sum of the output AS STORED, and everything the launch must leave alone"""
    dtype, c, px, res_mode, relu = case["dtype"], case["c"], case["px"], case["res"], case["relu"]
    V, dims, name = vec_of(dtype), dims_of(case["px"]), case_name(case)
    cgs = c // V
    gen = torch.Generator().manual_seed(1000 + seed_no + 7 * c + px + 3 * res_mode + int(relu))
    st = _stream(dev)
    y = _in_map(gen, dev, dtype, dims, c, c + 8, 8)
    res = _in_map(gen, dev, dtype, dims, c, 2 * c, 0) if res_mode else None
    out = y if case["alias"] else _out_map(dev, dtype, dims, c, c + V, V)
    scale, shift = _coef(gen, dev, c, "scale"), _coef(gen, dev, c, "shift")
    rs, rb = (_coef(gen, dev, c, "scale"), _coef(gen, dev, c, "shift")) if res_mode == 2 else (None, None)
    bits = torch.full((px * cgs + GUARD,), BYTE_SENT, dtype=torch.uint8, device=dev) if relu else None
    mp = case["sums"]
    sums = _sentbuf(mp * c * 2, dev) if mp else None
    y0, out0, res0 = y.buf.clone(), out.buf.clone(), (res.buf.clone() if res is not None else None)
    nparts = 0
    if mp:
        run, nparts = be.bn_apply(y, scale, shift, None, None, None, True, out, relu_bits=bits, out_sums=sums, max_parts=mp)
    else:
        run = be.bn_apply(y, scale, shift, res, rs, rb, relu, out, relu_bits=bits)
    run(st)
    _sync(dev)

    v, a, amb = apply_ref(_view(y, y0), scale, shift, _view(res, res0) if res is not None else None, rs, rb)
    vs = []
    if relu:
        r, alt = v.clamp_min(0), torch.where(v > 0, torch.zeros_like(v), v)
        vs.append(compare(f"out {name}", out.view5(), r, a, 4, dtype, kind_of(dtype), alt=alt, alt_mask=amb))
        want, am = (v > 0).reshape(px, c), amb.reshape(px, c)
        got = relu_bits_unpack(bits, px, c, V)
        packed = relu_bits_pack(torch.where(am, got, want), V)          # the reference sign except at ambiguous elements
        vs.append(Exact(f"relu_bits {name}", torch.equal(bits[: px * cgs], packed), f"{int(am.sum())} ambiguous of {am.numel()}"))
        vs.append(guard_ok(f"relu_bits tail {name}", [bits], [px * cgs]))
        vs.append(amb_share(name, amb))
    else:
        vs.append(compare(f"out {name}", out.view5(), v, a, 4, dtype, kind_of(dtype)))
    vs.append(untouched(f"out padding {name}", out, out0))
    if not case["alias"]:
        vs.append(same(f"y kept {name}", y.buf, y0))
    if res is not None:
        vs.append(same(f"res kept {name}", res.buf, res0))
    if mp:
        rows = sums[: mp * c * 2].view(mp, c, 2)
        vs.append(Exact(f"nparts {name}", 1 <= nparts <= mp, f"{nparts} of at most {mp}"))
        rest_ok = bool((rows[nparts:] == SENT).all()) and bool((sums[mp * c * 2:] == SENT).all())
        vs.append(Exact(f"rows past nparts {name}", rest_ok, f"{mp - nparts} rows and the guard"))
        vs.append(Exact(f"out_sums component 1 {name}", bool((rows[:nparts, :, 1] == 0).all()), "exactly 0"))
        # against the map the kernel WROTE (rounded to its dtype), not the pre-rounding value: that is what the contract says
        stored = out.view5().to(F64).reshape(px, c)
        vs.append(compare(f"out_sums {name}", rows[:nparts, :, 0].double().sum(0), stored.sum(0), stored.abs().sum(0), px, F32,
                          "sum_f32"))
    return vs


# ----------------------------------------------------------------------------- sfk_bn_bwd_apply
def bwd_apply_ref(da, y, mask, mean, invstd, coef):
    """dy = c0 (dz - c1 - x_hat c2), dz = da * mask, x_hat = (y - mean) invstd; coef (c, 3)"""
    d, yv, mu, is_, cf = da.to(F64), y.to(F64), mean.to(F64), invstd.to(F64), coef.to(F64)
    dz = d * mask.to(F64)
    r = cf[:, 0] * (dz - cf[:, 1] - (yv - mu) * is_ * cf[:, 2])
    a = cf[:, 0].abs() * (dz.abs() + cf[:, 1].abs() + (yv.abs() + mu.abs()) * is_.abs() * cf[:, 2].abs())
    return r, a


def _bwd_apply_cases():
    return [dict(dtype=dtype, cm=cm, c=cm * vec_of(dtype), px=px, mask=mask, inplace=inplace)
            for dtype in (BF16, F32) for cm in CMULS for mask in (0, 1, 2) for inplace in (False, True)
            for px in _apply_px(cm * vec_of(dtype), dtype)]


BWD_APPLY_CASES = _bwd_apply_cases()


def _bwd_inputs(gen, dev, c):
    """coef, mean, invstd drawn independently of each other (no chained reduce: a swapped c1 / c2 cannot cancel)"""
    mean, invstd = _coef(gen, dev, c, "shift"), (0.5 + 1.5 * torch.rand(c, generator=gen)).to(dev)
    coef = torch.stack([(torch.rand(c, generator=gen) + 0.5) * (1 - 2 * (torch.rand(c, generator=gen) < 0.3).float()),
                        0.1 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)], 1).to(dev)
    return mean, invstd, coef


def check_bwd_apply(be, dev, case, seed_no: int = 0) -> List:
    dtype, c, px, mask, inplace = case["dtype"], case["c"], case["px"], case["mask"], case["inplace"]
    V, dims, name = vec_of(dtype), dims_of(px), case_name(case)
    gen = torch.Generator().manual_seed(2000 + seed_no + 7 * c + px + 3 * mask + int(inplace))
    st = _stream(dev)
    da = _in_map(gen, dev, dtype, dims, c, c + 8, 8)
    y = _in_map(gen, dev, dtype, dims, c, 2 * c, c)
    ms = _in_map(gen, dev, dtype, dims, c, c + V, 0) if mask == 2 else None
    dy = da if inplace else _out_map(dev, dtype, dims, c, c + 2 * V, V)
    mean, invstd, coef = _bwd_inputs(gen, dev, c)
    scale, shift = (_coef(gen, dev, c, "scale"), _coef(gen, dev, c, "shift")) if mask == 1 else (None, None)
    da0, y0, dy0 = da.buf.clone(), y.buf.clone(), dy.buf.clone()
    be.bn_bwd_apply(da, y, ms, mean, invstd, scale, shift, mask == 1, coef.reshape(-1), dy)(st)
    _sync(dev)
    vs = []
    if mask == 1:
        v, _, amb = apply_ref(_view(y, y0), scale, shift)
        m = v > 0
        r, a = bwd_apply_ref(_view(da, da0), _view(y, y0), m, mean, invstd, coef)
        alt, _ = bwd_apply_ref(_view(da, da0), _view(y, y0), ~m, mean, invstd, coef)
        vs.append(compare(f"dy {name}", dy.view5(), r, a, 4, dtype, kind_of(dtype), alt=alt, alt_mask=amb))
        vs.append(amb_share(name, amb))
    else:
        m = (ms.view5() > 0) if mask == 2 else torch.ones_like(_view(da, da0), dtype=torch.bool)
        r, a = bwd_apply_ref(_view(da, da0), _view(y, y0), m, mean, invstd, coef)
        vs.append(compare(f"dy {name}", dy.view5(), r, a, 4, dtype, kind_of(dtype)))
    vs.append(untouched(f"dy padding {name}", dy, dy0))
    vs.append(same(f"y kept {name}", y.buf, y0))
    if not inplace:
        vs.append(same(f"da kept {name}", da.buf, da0))
    return vs


# ----------------------------------------------------------------------------- the two loops no small case reaches
def _halves(m: FMap, cut: int):
    px = m.pixels
    return (FMap(m.buf, 1, 1, 1, cut, m.c, m.ld, m.c_off), FMap(m.buf[cut * m.ld:], 1, 1, 1, px - cut, m.c, m.ld, m.c_off))


CAP_C = 1024
CAP_PX = SPAN_U * GRID_CAP + 1030      # fp32, 256 channel groups: rows_b = 1, 65,793 spans on 65,535 blocks


def check_grid_cap_apply(be, dev, px: int = CAP_PX, c: int = CAP_C) -> List:
    """sfk_bn_apply (ReLU, plain residual, bitmap) over the whole map in ONE launch -- more spans than the grid has blocks, so
    the loop takes its second trip -- bit for bit against two launches over the map's pixel halves, each under the cap"""
    st = _stream(dev)
    g = torch.Generator(device=dev).manual_seed(31)
    rn = lambda: torch.randn(px * c, generator=g, device=dev)
    y, res = FMap(rn(), 1, 1, 1, px, c), FMap(rn(), 1, 1, 1, px, c)
    scale, shift = torch.rand(c, generator=g, device=dev) + 0.5, 0.3 * torch.randn(c, generator=g, device=dev)
    one, two = FMap(torch.full((px * c,), SENT, device=dev), 1, 1, 1, px, c), FMap(torch.full((px * c,), SENT, device=dev), 1, 1, 1, px, c)
    cgs = c // 4
    b1 = torch.full((px * cgs,), BYTE_SENT, dtype=torch.uint8, device=dev)
    b2 = b1.clone()
    be.bn_apply(y, scale, shift, res, None, None, True, one, relu_bits=b1)(st)
    cut = px // 2
    for yh, rh, oh, bh in zip(_halves(y, cut), _halves(res, cut), _halves(two, cut), (b2, b2[cut * cgs:])):
        be.bn_apply(yh, scale, shift, rh, None, None, True, oh, relu_bits=bh)(st)
    _sync(dev)
    spans = (px + SPAN_U - 1) // SPAN_U
    return [Exact(f"bn_apply px {px} out", torch.equal(_bits(one.buf), _bits(two.buf)), f"{spans} spans, one launch == two halves"),
            Exact(f"bn_apply px {px} written", bool((one.buf != SENT).all()), "no sentinel left"),
            Exact(f"bn_apply px {px} relu_bits", torch.equal(b1, b2), "one launch == two halves")]


def check_grid_cap_bwd_apply(be, dev, px: int = CAP_PX, c: int = CAP_C) -> List:
    """sfk_bn_bwd_apply (mask recomputed from y) the same way"""
    st = _stream(dev)
    g = torch.Generator(device=dev).manual_seed(32)
    rn = lambda: torch.randn(px * c, generator=g, device=dev)
    da, y = FMap(rn(), 1, 1, 1, px, c), FMap(rn(), 1, 1, 1, px, c)
    scale, shift = torch.rand(c, generator=g, device=dev) + 0.5, 0.3 * torch.randn(c, generator=g, device=dev)
    mean, invstd = 0.3 * torch.randn(c, generator=g, device=dev), torch.rand(c, generator=g, device=dev) + 0.5
    coef = torch.randn(c * 3, generator=g, device=dev)
    one, two = FMap(torch.full((px * c,), SENT, device=dev), 1, 1, 1, px, c), FMap(torch.full((px * c,), SENT, device=dev), 1, 1, 1, px, c)
    be.bn_bwd_apply(da, y, None, mean, invstd, scale, shift, True, coef, one)(st)
    cut = px // 2
    for dh, yh, oh in zip(_halves(da, cut), _halves(y, cut), _halves(two, cut)):
        be.bn_bwd_apply(dh, yh, None, mean, invstd, scale, shift, True, coef, oh)(st)
    _sync(dev)
    return [Exact(f"bn_bwd_apply px {px} dy", torch.equal(_bits(one.buf), _bits(two.buf)), "one launch == two halves"),
            Exact(f"bn_bwd_apply px {px} written", bool((one.buf != SENT).all()), "no sentinel left")]


STREAM_C = 64


def streamed_px(mb: int) -> int:
    """the first bf16 pixel count at c = 64 whose map reaches `mb` MB, plus 37"""
    return -((-(mb << 20)) // (STREAM_C * 2)) + 37


def check_streamed_bwd_apply(be, dev, px: int, chunk: int = 1 << 17) -> List:
    """one bf16 sfk_bn_bwd_apply launch (mask recomputed from y) held to float64, the reference evaluated in pixel chunks"""
    c, dtype = STREAM_C, BF16
    st = _stream(dev)
    g = torch.Generator(device=dev).manual_seed(33)
    da = FMap(torch.randn(px * c, generator=g, device=dev).to(dtype), 1, 1, 1, px, c)
    y = FMap(torch.randn(px * c, generator=g, device=dev).to(dtype), 1, 1, 1, px, c)
    dy = FMap(torch.full((px * c + GUARD,), SENT, dtype=dtype, device=dev), 1, 1, 1, px, c)
    gc = torch.Generator().manual_seed(34)
    mean, invstd, coef = _bwd_inputs(gc, dev, c)
    scale, shift = _coef(gc, dev, c, "scale"), _coef(gc, dev, c, "shift")
    be.bn_bwd_apply(da, y, None, mean, invstd, scale, shift, True, coef.reshape(-1), dy)(st)
    _sync(dev)
    vs, n_amb = [], 0
    for p0 in range(0, px, chunk):
        sl = slice(p0 * c, min(px, p0 + chunk) * c)
        dv, yv, ov = da.buf[sl].view(-1, c), y.buf[sl].view(-1, c), dy.buf[sl].view(-1, c)
        v, _, amb = apply_ref(yv, scale, shift)
        r, a = bwd_apply_ref(dv, yv, v > 0, mean, invstd, coef)
        alt, _ = bwd_apply_ref(dv, yv, ~(v > 0), mean, invstd, coef)
        vs.append(compare(f"dy streamed pixels {p0}+", ov, r, a, 4, dtype, "map_bf16", alt=alt, alt_mask=amb))
        n_amb += int(amb.sum())
    vs.append(Exact("ambiguous ReLU signs streamed", n_amb < AMB_CAP * px * c, f"{n_amb} of {px * c}"))
    vs.append(guard_ok("dy guard streamed", [dy.buf], [px * c]))
    return vs


# ----------------------------------------------------------------------------- finalize kernels
def bn_derived(mu, a_mu, var_raw, a_var, count, gamma, beta, eps, momentum, rm, rv) -> Dict:
    """everything sfk_bn_finalize / sfk_bn_tail_fwd derive from (mean, var): name -> (value, a), float64.
    eps and momentum are the float32 values the C ABI carries.  The derivations:
      invstd = (var + eps)^-1/2, d invstd / d var = -invstd^3 / 2: an error e in var moves invstd by invstd^3 e / 2, so
          a(invstd) = |invstd| + invstd^3 a(var) / 2             (its own rounding, and var's error through the derivative)
      scale = gamma invstd                    ->  a(scale) = |gamma| a(invstd)
      shift = beta - mean scale               ->  a(shift) = |beta| + |mean| a(scale) + |scale| a(mean)
      running_mean' = (1 - m) rm + m mean     ->  a = |(1 - m) rm| + m a(mean)
      running_var'  = (1 - m) rv + m var u, u = count / (count - 1) (1 at count = 1)  ->  a = |(1 - m) rv| + m u a(var)"""
    eps, mom = f32(eps), f32(momentum)
    g_, b_ = gamma.to(F64), beta.to(F64)
    var = var_raw.clamp_min(0.0)
    is_ = (var + eps) ** -0.5
    a_is = is_ + 0.5 * is_ ** 3 * a_var
    sc, a_sc = g_ * is_, g_.abs() * a_is
    sh, a_sh = b_ - mu * sc, b_.abs() + mu.abs() * a_sc + sc.abs() * a_mu
    out = dict(mean=(mu, a_mu), invstd=(is_, a_is), scale=(sc, a_sc), shift=(sh, a_sh), var=(var, a_var))
    if rm is not None:
        u = count / (count - 1.0) if count > 1 else 1.0
        out["rm"] = ((1 - mom) * rm.to(F64) + mom * mu, ((1 - mom) * rm.to(F64)).abs() + mom * a_mu)
        out["rv"] = ((1 - mom) * rv.to(F64) + mom * var * u, ((1 - mom) * rv.to(F64)).abs() + mom * u * a_var)
    return out


def finalize_ref(s1, a1, s2, a2, count, gamma, beta, eps, momentum, rm, rv) -> Dict:
    """mean = s1 / count, var = s2 / count - mean^2 (clamped at 0): a(mean) = a1 / count, a(var) = a2 / count + mean^2"""
    mu = s1 / count
    return bn_derived(mu, a1 / count, s2 / count - mu * mu, a2 / count + mu * mu, count, gamma, beta, eps, momentum, rm, rv)


def bwd_finalize_ref(s1, a1, s2, a2, count, gamma, invstd, dgamma0, dbeta0) -> Dict:
    out = dict(coef0=(gamma.to(F64) * invstd.to(F64), (gamma.to(F64) * invstd.to(F64)).abs()),
               coef1=(s1 / count, a1 / count), coef2=(s2 / count, a2 / count))
    if dgamma0 is not None:
        out["dgamma"] = (dgamma0.to(F64) + s2, dgamma0.to(F64).abs() + a2)
    if dbeta0 is not None:
        out["dbeta"] = (dbeta0.to(F64) + s1, dbeta0.to(F64).abs() + a1)
    return out


def eval_coeffs_ref(gamma, beta, rm, rv, eps):
    """invstd = (rv + eps)^-1/2 with the fp32 sum rv + eps behind it: a(rv + eps) = rv + eps through -invstd^3 / 2 is
    invstd / 2, so a(invstd) = 3/2 invstd; scale and shift as in bn_derived (running_mean is an exact input)"""
    g_, b_, m_ = gamma.to(F64), beta.to(F64), rm.to(F64)
    is_ = (rv.to(F64) + f32(eps)) ** -0.5
    a_is = 1.5 * is_
    sc, a_sc = g_ * is_, g_.abs() * a_is
    return dict(scale=(sc, a_sc), shift=(b_ - m_ * sc, b_.abs() + m_.abs() * a_sc))


def _fin_cases():
    out = []
    for c in (2, 6, 130):
        for nparts, ws in ((1, False), (255, False), (257, False), (4097, False), (4097, True)):
            for count_one in (False, True):
                for running in ((True, False) if nparts in (1, 257) else (True,)):
                    out.append(dict(c=c, nparts=nparts, ws=ws, count_one=count_one, running=running))
    out.append(dict(c=8, nparts=50176, ws=True, count_one=False, running=True))
    return out


FIN_CASES = _fin_cases()
EVAL_C = (1, 63, 65, 130)
CLAMP_CH = 1                   # the channel whose sums make var slightly negative


def fin_name(case) -> str:
    return (f"c{case['c']}-rows{case['nparts']}{'-ws' if case['ws'] else ''}{'-count1' if case['count_one'] else ''}"
            f"{'' if case['running'] else '-norunning'}")


def fin_partials(case, gen):
    """[nparts][c][2] float32 and the count.  count = 4 nparts: row i = (sum, sum of squares) of four samples of a channel
    with its own mean and spread; channel CLAMP_CH is the constant 3 with the squares short by 2^-20, so that
    var = s2 / count - mean^2 = -9 * 2^-20 and clamps.  count = 1: rows whose sums keep var positive."""
    c, nparts = case["c"], case["nparts"]
    if case["count_one"]:
        p0 = 0.1 * torch.randn(nparts, c, generator=gen, dtype=F64) / nparts
        p1 = (0.5 + torch.rand(nparts, c, generator=gen, dtype=F64)) / nparts
        return torch.stack([p0, p1], 2).float(), 1
    mu, sd = torch.randn(c, generator=gen, dtype=F64), 0.5 + torch.rand(c, generator=gen, dtype=F64)
    x = mu + sd * torch.randn(nparts, 4, c, generator=gen, dtype=F64)
    p = torch.stack([x.sum(1), (x * x).sum(1)], 2)
    p[:, CLAMP_CH, 0], p[:, CLAMP_CH, 1] = 12.0, 36.0 * (1.0 - 2.0 ** -20)
    return p.float(), 4 * nparts


def fold_k(case) -> int:
    """with a workspace and more rows than the finalize launch folds itself (csrc/bn.hip fold_partials), the first level
    leaves up to SFK_BN_FOLD_ROWS float32 row sums: the longest fp32 chain behind a value; otherwise the sums stay in double"""
    big = case["nparts"] > 4096 or case["nparts"] * case["c"] > 4096 * 128
    return BN_FOLD_ROWS if (case["ws"] and big) else 1


def check_finalize(be, dev, case, seed_no: int = 0) -> List:
    """sfk_bn_finalize, then sfk_bn_bwd_finalize on the same rows read as (sum dz, sum dz x_hat)"""
    c, nparts, name = case["c"], case["nparts"], fin_name(case)
    gen = torch.Generator().manual_seed(3000 + seed_no + 11 * c + nparts + int(case["count_one"]))
    st = _stream(dev)
    p, count = fin_partials(case, gen)
    parts = p.reshape(-1).to(dev)
    rn = lambda: torch.randn(c, generator=gen)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(dev), (0.3 * rn()).to(dev)
    ws = _sentbuf(BN_FOLD_ROWS * c * 2, dev) if case["ws"] else None
    mean, invstd, scale, shift = (_sentbuf(c, dev) for _ in range(4))
    rm0, rv0 = rn().to(dev), (torch.rand(c, generator=gen) + 0.5).to(dev)
    running = case["running"]
    rm, rv = (_vecbuf(rm0, dev), _vecbuf(rv0, dev)) if running else (None, None)
    nbt = torch.tensor([41], dtype=torch.int64, device=dev) if running else None
    be.bn_finalize(parts, nparts, c, count, gamma, beta, EPS, MOMENTUM, rm, rv, nbt, mean, invstd, scale, shift, ws)(st)
    invstd_in = (torch.rand(c, generator=gen) + 0.5).to(dev)
    dg0, db0 = rn().to(dev), rn().to(dev)
    dgamma, dbeta = (_vecbuf(dg0, dev), _vecbuf(db0, dev)) if running else (None, None)
    coef = _sentbuf(c * 3, dev)
    ws2 = _sentbuf(BN_FOLD_ROWS * c * 2, dev) if case["ws"] else None
    be.bn_bwd_finalize(parts, nparts, c, count, gamma, invstd_in, dgamma, dbeta, coef, ws2)(st)
    _sync(dev)

    P = parts.view(nparts, c, 2).double()
    s1, s2, a1, a2 = P[:, :, 0].sum(0), P[:, :, 1].sum(0), P[:, :, 0].abs().sum(0), P[:, :, 1].abs().sum(0)
    K = fold_k(case)
    ref = finalize_ref(s1, a1, s2, a2, count, gamma, beta, EPS, MOMENTUM, rm0 if running else None, rv0 if running else None)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, rm=rm, rv=rv)
    vs = [Exact(f"var clamps {name}", case["count_one"] or float((s2 / count - (s1 / count) ** 2)[CLAMP_CH]) < 0, f"channel {CLAMP_CH}")]
    for k in ("mean", "invstd", "scale", "shift") + (("rm", "rv") if running else ()):
        vs.append(compare(f"{k} {name}", got[k][:c], ref[k][0], ref[k][1], max(K, 2 if k in ("rm", "rv") else 1), F32, "sum_f32"))
    if running:
        vs.append(Exact(f"num_batches_tracked {name}", int(nbt[0]) == 42, f"{int(nbt[0])} want 42"))
    bref = bwd_finalize_ref(s1, a1, s2, a2, count, gamma, invstd_in, dg0 if running else None, db0 if running else None)
    cf = coef[: c * 3].view(c, 3)
    for j in range(3):
        vs.append(compare(f"coef{j} {name}", cf[:, j], *bref[f"coef{j}"], K, F32, "sum_f32"))
    if running:
        vs.append(compare(f"dgamma {name}", dgamma[:c], *bref["dgamma"], max(K, 2), F32, "sum_f32"))
        vs.append(compare(f"dbeta {name}", dbeta[:c], *bref["dbeta"], max(K, 2), F32, "sum_f32"))
    bufs = [mean, invstd, scale, shift, coef] + ([rm, rv, dgamma, dbeta] if running else [])
    used = [c, c, c, c, c * 3] + ([c] * 4 if running else [])
    if case["ws"]:
        bufs, used = bufs + [ws, ws2], used + [BN_FOLD_ROWS * c * 2] * 2
    vs.append(guard_ok(f"guards {name}", bufs, used))
    vs.append(same(f"partials kept {name}", parts, p.reshape(-1).to(dev)))
    return vs


def check_eval_coeffs(be, dev, c: int) -> List:
    gen = torch.Generator().manual_seed(3500 + c)
    rn = lambda: torch.randn(c, generator=gen)
    gamma, beta, rm = rn().to(dev), rn().to(dev), rn().to(dev)
    rv = (torch.rand(c, generator=gen) + 0.5)
    rv[0] = 0.0                                      # invstd = 1 / sqrt(eps)
    rv = rv.to(dev)
    scale, shift = _sentbuf(c, dev), _sentbuf(c, dev)
    be.bn_eval_coeffs(gamma, beta, rm, rv, EPS, c, scale, shift)(_stream(dev))
    _sync(dev)
    ref = eval_coeffs_ref(gamma, beta, rm, rv, EPS)
    return [compare(f"scale c{c}", scale[:c], *ref["scale"], 1, F32, "sum_f32"),
            compare(f"shift c{c}", shift[:c], *ref["shift"], 1, F32, "sum_f32"),
            guard_ok(f"guards c{c}", [scale, shift], [c, c])]


# ----------------------------------------------------------------------------- max-pool
POOL_WINDOWS = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 3, 2))
POOL_HW = ((1, 1), (3, 3), (6, 4), (7, 5), (4, 7))


def _pool_cases():
    out = []
    for dtype in (BF16, F32):
        for k, s, p in POOL_WINDOWS:
            for h, w in POOL_HW:
                if h + 2 * p >= k and w + 2 * p >= k:
                    out.append(dict(dtype=dtype, k=k, s=s, p=p, h=h, w=w, fill="mixed"))
            out.append(dict(dtype=dtype, k=k, s=s, p=p, h=7, w=5, fill="negative"))     # padding must lose
        out.append(dict(dtype=dtype, k=3, s=2, p=1, h=7, w=5, fill="nan"))
    return out


POOL_CASES = _pool_cases()


def pool_name(case) -> str:
    return f"{tag_of(case['dtype'])}-k{case['k']}s{case['s']}p{case['p']}-{case['h']}x{case['w']}-{case['fill']}"


def pool_windows_per_pixel(k: int, s: int) -> int:
    """how many windows one input pixel can lie in: the terms of one backward sum"""
    return (-(-k // s)) ** 2


def torch_pool(x5: torch.Tensor, k: int, s: int, p: int):
    """F.max_pool3d with indices on the CPU -- torch's rule: start from the first tap inside the frame, replace on
    (value > maximum) or isnan(value) -- as (values, argmax = kh * k + kw) in the (N,T,Ho,Wo,C) layout"""
    x = x5.detach().to("cpu", F64).permute(0, 4, 1, 2, 3).contiguous()
    h, w = x.shape[3], x.shape[4]
    val, idx = torch.nn.functional.max_pool3d(x, (1, k, k), (1, s, s), (0, p, p), return_indices=True)
    ho, wo = val.shape[3], val.shape[4]
    hi, wi = (idx % (h * w)) // w, idx % w
    kh = hi - (torch.arange(ho).view(1, 1, 1, ho, 1) * s - p)
    kw = wi - (torch.arange(wo).view(1, 1, 1, 1, wo) * s - p)
    return val.permute(0, 2, 3, 4, 1), (kh * k + kw).to(torch.uint8).permute(0, 2, 3, 4, 1)


def pool_input(case, gen) -> torch.Tensor:
    """(N,T,H,W,C) float64 values on a few levels, so that ties are common; both signs unless the case says otherwise"""
    n, t, c = case.get("n", 2), case.get("t", 2), case.get("cg", 3) * vec_of(case["dtype"])     # (tests/tuned_tables.py sets them)
    q = (1.5 * torch.randn(n, t, case["h"], case["w"], c, generator=gen, dtype=F64)).round().clamp(-4, 4)
    if case["fill"] == "negative":
        q = -1.0 - q.abs()
    if case["fill"] == "nan":
        q[torch.rand(q.shape, generator=gen) < 0.06] = float("nan")
    return q


def _nan_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def check_pool(be, dev, case, seed_no: int = 0) -> List:
    """forward values and argmax bytes exactly; the backward, routed by the backend's OWN argmax, against float64"""
    dtype, k, s, p, h, w = case["dtype"], case["k"], case["s"], case["p"], case["h"], case["w"]
    V, name = vec_of(dtype), pool_name(case)
    gen = torch.Generator().manual_seed(4000 + seed_no + 13 * k + 5 * s + p + 31 * h + w)
    st = _stream(dev)
    q = pool_input(case, gen)
    n, t, c = q.shape[0], q.shape[1], q.shape[4]
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x = _in_map(gen, dev, dtype, (n, t, h, w), c, c + V, V)
    x.view5().copy_(q.to(dtype))
    y = _out_map(dev, dtype, (n, t, ho, wo), c, c + 2 * V, 0)
    opx = n * t * ho * wo
    argmax = torch.full((opx * c + GUARD,), BYTE_SENT, dtype=torch.uint8, device=dev)
    x0, y0 = x.buf.clone(), y.buf.clone()
    be.maxpool_fwd(x, y, argmax, k, s, p)(st)
    d_out = _in_map(gen, dev, dtype, (n, t, ho, wo), c, c + V, 0)
    dx = _out_map(dev, dtype, (n, t, h, w), c, c + 2 * V, V)
    d0, dx0 = d_out.buf.clone(), dx.buf.clone()
    be.maxpool_bwd(d_out, argmax, dx, k, s, p)(st)
    _sync(dev)
    if case["fill"] == "nan":
        best, arg = (z.to(dev) for z in torch_pool(x.view5(), k, s, p))
    else:
        best, arg = ref64.maxpool_fwd(x.view5().to(F64), k, s, p)
    got_arg = argmax[: opx * c].view(n, t, ho, wo, c)
    vs = [Exact(f"pooled values {name}", _nan_equal(y.view5().to(F64), best), f"{opx * c} values, first-maximum rule"),
          Exact(f"argmax {name}", torch.equal(got_arg, arg), f"{opx * c} bytes"),
          guard_ok(f"argmax tail {name}", [argmax], [opx * c]),
          untouched(f"y padding {name}", y, y0), same(f"x kept {name}", x.buf, x0)]
    r = ref64.maxpool_bwd(d_out.view5(), got_arg, h, w, k, s, p)
    a = ref64.maxpool_bwd(d_out.view5().abs(), got_arg, h, w, k, s, p)
    vs.append(compare(f"dx {name}", dx.view5(), r, a, pool_windows_per_pixel(k, s), dtype, kind_of(dtype)))
    vs += [untouched(f"dx padding {name}", dx, dx0), same(f"d_out kept {name}", d_out.buf, d0)]
    return vs


# ----------------------------------------------------------------------------- the block tail's small algebra
def tail_fwd_ref(G, g, n, W, gamma, beta, eps, momentum, rm, rv) -> Dict:
    """sfk_bn_tail_fwd from G = a^T a, g = 1^T a and n as the kernel receives them: name -> (value, a).
    T = W G (an fp32 chain of c terms); mean = W g / n; var = W Gc W^T over the centred Gc = G / n - (g / n)(g / n)^T -- the
    contract forms Gc in double, so the terms of the variance are the centred products: a(var) = |W| |Gc| |W|^T;
    wd = (scale (x) W)^T  ->  a(wd) = a(scale) |W|"""
    G, g, W = G.to(F64), g.to(F64), W.to(F64)
    gb = g / n
    Gc = G / n - torch.outer(gb, gb)
    mu, a_mu = W @ g / n, W.abs() @ g.abs() / n
    var_raw, a_var = ((W @ Gc) * W).sum(1), ((W.abs() @ Gc.abs()) * W.abs()).sum(1)
    out = bn_derived(mu, a_mu, var_raw, a_var, n, gamma, beta, eps, momentum, rm, rv)
    out["t"] = (W @ G, W.abs() @ G.abs())
    out["wd"] = ((out["scale"][0][:, None] * W).t(), (out["scale"][1][:, None] * W.abs()).t())
    return out


def tail_bwd_ref(R, s, a_s, g, n, T, W, gamma, mean, invstd, dgamma0, dbeta0, dw0) -> Dict:
    """sfk_bn_tail_bwd: name -> (value, a).  With sdy = sum_ci W R (per output channel, in double), s = sum dz:
      sxh = invstd (sdy - mean s)                      a(sxh) = |invstd| (a(sdy) + |mean| a(s))
      A = gamma invstd, c1 = s / n, c2 = sxh / n
      B = -A c2 invstd                                 a(B) = |A invstd| a(sxh) / n
      C = A (c2 invstd mean - c1)                      a(C) = |A| (|invstd mean| a(sxh) / n + a(s) / n)
      dW += A R + B T + C (x) g  (fp32, from the ROUNDED coefficients: their error comes through |T| and |g|)
                                                       a(dW) = |dW0| + |A R| + a(B) |T| + a(C) |g|
      m = W^T diag(B) W  (an fp32 chain of cout terms) a(m) = |W|^T diag(a(B)) |W|
      bias = C W                                       a(bias) = a(C) |W|"""
    R, s, g, T, W = R.to(F64), s.to(F64), g.to(F64), T.to(F64), W.to(F64)
    mu, is_, gam = mean.to(F64), invstd.to(F64), gamma.to(F64)
    sdy, a_sdy = (W * R).sum(1), (W * R).abs().sum(1)
    sxh, a_sxh = is_ * (sdy - mu * s), is_.abs() * (a_sdy + mu.abs() * a_s)
    A = gam * is_
    c1, c2 = s / n, sxh / n
    B, a_B = -A * c2 * is_, (A * is_).abs() * a_sxh / n
    C, a_C = A * (c2 * is_ * mu - c1), A.abs() * ((is_ * mu).abs() * a_sxh / n + a_s / n)
    dw = dw0.to(F64) + A[:, None] * R + B[:, None] * T + C[:, None] * g[None, :]
    a_dw = dw0.to(F64).abs() + (A[:, None] * R).abs() + a_B[:, None] * T.abs() + a_C[:, None] * g.abs()[None, :]
    return dict(dgamma=(dgamma0.to(F64) + sxh, dgamma0.to(F64).abs() + a_sxh), dbeta=(dbeta0.to(F64) + s, dbeta0.to(F64).abs() + a_s),
                A=(A, A.abs()), B=(B, a_B), C=(C, a_C), dw=(dw, a_dw),
                m=(W.t() @ (B[:, None] * W), W.abs().t() @ (a_B[:, None] * W.abs())), bias=(C @ W, a_C @ W.abs()))


TAIL_SHAPES = ((8, 4), (24, 36), (40, 20), (264, 72), (512, 12))
TAIL_PARTS = ((1, 200), (63, 65), (65, 63), (200, 1))          # (a_nparts, nparts): around the 64-lane stride of the row folds
TAIL_PX = 401
MD_RATIO = 1e3
MD_PX = 4099                   # no power of two: 1 / n and the column means g / n do not come out exact in fp32


def _tail_cases():
    out, i = [], 0
    for c, cout in TAIL_SHAPES:
        for wdt in (F32, BF16):
            for a_np, np_ in TAIL_PARTS:
                out.append(dict(c=c, cout=cout, wdt=wdt, a_np=a_np, np=np_, wd=i % 2 == 0, running=(i // 2) % 2 == 0, md=False))
                i += 1
    # mean-dominated channels: mean^2 / var > 1e3 (tests/test_gpu_kernels.py test_bottleneck_tail_variance_of_mean_dominated_channels)
    out.append(dict(c=64, cout=32, wdt=F32, a_np=1, np=1, wd=True, running=True, md=True))
    return out


TAIL_CASES = _tail_cases()


def tail_name(case) -> str:
    return (f"c{case['c']}-cout{case['cout']}-{tag_of(case['wdt'])}-rows{case['a_np']}+{case['np']}{'-wd' if case['wd'] else ''}"
            f"{'' if case['running'] else '-norunning'}{'-mean-dominated' if case['md'] else ''}")


def _part_rows(x: torch.Tensor, nparts: int) -> torch.Tensor:
    """[nparts][cols][2] float32: component 0 = the column sums of x's row chunks, component 1 = junk no kernel may read"""
    rows = torch.stack([ch.sum(0) for ch in torch.tensor_split(x, nparts)], 0)
    return torch.stack([rows, torch.full_like(rows, 777.0)], 2).float()


def check_tail(be, dev, case, seed_no: int = 0) -> List:
    """sfk_bn_tail_fwd and sfk_bn_tail_bwd called directly.  `a`, the filter and dz are drawn in float64; G = a^T a, the partial
    rows, R = dz^T a (and, for the backward, g, T, mean, invstd) are rounded ONCE to fp32: these are the kernels' inputs, and the
    reference starts from the same fp32 numbers"""
    c, cout, wdt, a_np, np_, name = case["c"], case["cout"], case["wdt"], case["a_np"], case["np"], tail_name(case)
    gen = torch.Generator().manual_seed(5000 + seed_no + 17 * c + cout + a_np)
    st = _stream(dev)
    px = MD_PX if case["md"] else TAIL_PX
    if case["md"]:
        a = torch.randn(px, c, generator=gen, dtype=F64) + MD_RATIO ** 0.5 * 3.0
        W64 = torch.rand(cout, c, generator=gen, dtype=F64) * 0.2 + 0.05
    else:
        a = (torch.randn(px, c, generator=gen, dtype=F64) + 0.5).clamp_min(0)
        W64 = torch.randn(cout, c, generator=gen, dtype=F64) * c ** -0.5
    w = W64.to(wdt).reshape(-1).to(dev)
    W = w.view(cout, c).double()
    gram = (a.t() @ a).float().reshape(-1).to(dev)
    asums = _part_rows(a, a_np).reshape(-1).to(dev)
    gamma, beta = (torch.rand(cout, generator=gen) + 0.5).to(dev), (0.3 * torch.randn(cout, generator=gen)).to(dev)
    rm0, rv0 = torch.randn(cout, generator=gen).to(dev), (torch.rand(cout, generator=gen) + 0.5).to(dev)
    running = case["running"]
    rm, rv = (_vecbuf(rm0, dev), _vecbuf(rv0, dev)) if running else (None, None)
    nbt = torch.tensor([41], dtype=torch.int64, device=dev) if running else None
    g = _sentbuf(c, dev)
    mean, invstd, scale, shift = (_sentbuf(cout, dev) for _ in range(4))
    t = _sentbuf(cout * c, dev)
    wd = _sentbuf(c * cout, dev, wdt) if case["wd"] else None
    be.bn_tail_fwd(gram, asums, a_np, px, g, c, w, cout, gamma, beta, EPS, MOMENTUM, rm, rv, nbt, mean, invstd, scale, shift, t, wd)(st)
    _sync(dev)
    rows = asums.view(a_np, c, 2)[:, :, 0].double()
    vs = [compare(f"g {name}", g[:c], rows.sum(0), rows.abs().sum(0), 1, F32, "sum_f32")]
    # mean and variance from the g the backend folded (held to the row sums just above): the kernel reads that fp32 vector
    ref = tail_fwd_ref(gram.view(c, c), g[:c], px, W, gamma, beta, EPS, MOMENTUM, rm0 if running else None, rv0 if running else None)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, rm=rm, rv=rv)
    for k in ("mean", "invstd", "scale", "shift") + (("rm", "rv") if running else ()):
        # the mean is folded in double; everything behind the variance has the fp32 chain of c centred products behind it
        vs.append(compare(f"{k} {name}", got[k][:cout], ref[k][0], ref[k][1], 1 if k == "mean" else (2 if k == "rm" else c), F32, "sum_f32"))
    vs.append(compare(f"t {name}", t[: cout * c].view(cout, c), *ref["t"], c, F32, "sum_f32"))
    if wd is not None:
        vs.append(compare(f"wd {name}", wd[: c * cout].view(c, cout), *ref["wd"], 1, wdt, kind_of(wdt)))
    if running:
        vs.append(Exact(f"num_batches_tracked {name}", int(nbt[0]) == 42, f"{int(nbt[0])} want 42"))
    bufs = [g, mean, invstd, scale, shift, t] + ([rm, rv] if running else []) + ([wd] if wd is not None else [])
    used = [c, cout, cout, cout, cout, cout * c] + ([cout, cout] if running else []) + ([c * cout] if wd is not None else [])
    vs.append(guard_ok(f"forward guards {name}", bufs, used))
    if case["md"]:
        # that test's bound, against the float64 variance of y = a W^T itself: one fp32 rounding of G's entries ~ n mean^2 is
        # 6e-8 mean^2 / var relative to the variance
        yv = a.to(dev) @ W.t()
        want_mu, want_var = yv.mean(0), yv.var(0, unbiased=False)
        ratio = want_mu ** 2 / want_var
        got_var = 1.0 / invstd[:cout].double() ** 2 - f32(EPS)
        err = float((got_var - want_var).abs().max() / want_var.abs().max())
        bound = 4 * 6e-8 * float(ratio.max()) + 1e-5
        vs.append(Exact(f"mean^2 / var {name}", float(ratio.min()) > MD_RATIO, f"{float(ratio.min()):.3g} .. {float(ratio.max()):.3g}"))
        vs.append(Exact(f"variance to float64 y {name}", err < bound, f"max-norm error {err:.3g}, bound {bound:.3g}"))
        return vs

    # ---- backward: every input from the float64 side, rounded once
    dz = torch.randn(px, cout, generator=gen, dtype=F64) * (torch.rand(px, cout, generator=gen) < 0.5) / px
    r_in = (dz.t() @ a).float().reshape(-1).to(dev)
    dzp = _part_rows(dz, np_).reshape(-1).to(dev)
    g_in = a.sum(0).float().to(dev)
    t_in = (W @ gram.view(c, c).double()).float().reshape(-1).contiguous()
    mean_in, invstd_in = ref["mean"][0].float(), ref["invstd"][0].float()
    dg0, db0 = torch.randn(cout, generator=gen).to(dev), torch.randn(cout, generator=gen).to(dev)
    dw0 = (0.1 * torch.randn(cout * c, generator=gen)).to(dev)
    dgamma, dbeta, dw = _vecbuf(dg0, dev), _vecbuf(db0, dev), _vecbuf(dw0, dev)
    m, bias, coef = _sentbuf(c * c, dev, wdt), _sentbuf(c, dev), _sentbuf(cout * 4, dev)
    be.bn_tail_bwd(r_in, dzp, np_, g_in, px, t_in, c, w, cout, gamma, mean_in, invstd_in, dgamma, dbeta, dw, m, bias, coef)(st)
    _sync(dev)
    srow = dzp.view(np_, cout, 2)[:, :, 0].double()
    b = tail_bwd_ref(r_in.view(cout, c), srow.sum(0), srow.abs().sum(0), g_in, px, t_in.view(cout, c), W, gamma, mean_in, invstd_in,
                     dg0, db0, dw0.view(cout, c))
    cf = coef[: cout * 4].view(cout, 4)
    vs += [compare(f"dgamma {name}", dgamma[:cout], *b["dgamma"], 2, F32, "sum_f32"),
           compare(f"dbeta {name}", dbeta[:cout], *b["dbeta"], 2, F32, "sum_f32"),
           compare(f"coef A {name}", cf[:, 0], *b["A"], 1, F32, "sum_f32"),
           compare(f"coef B {name}", cf[:, 1], *b["B"], 1, F32, "sum_f32"),
           compare(f"coef C {name}", cf[:, 2], *b["C"], 1, F32, "sum_f32"),
           Exact(f"coef[3] {name}", bool((cf[:, 3] == 0).all()), "exactly 0"),
           compare(f"dw {name}", dw[: cout * c].view(cout, c), *b["dw"], 4, F32, "sum_f32"),
           compare(f"m {name}", m[: c * c].view(c, c), *b["m"], cout, wdt, kind_of(wdt)),
           compare(f"bias {name}", bias[:c], *b["bias"], 1, F32, "sum_f32"),
           guard_ok(f"backward guards {name}", [dgamma, dbeta, dw, m, bias, coef], [cout, cout, cout * c, c * c, c, cout * 4])]
    return vs
