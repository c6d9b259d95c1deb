"""TEST INFRASTRUCTURE: the case table of the conv / filter-gradient edge audit (tests/test_conv_edges_cpu.py,
tests/test_gpu_conv_edges.py).  No GPU import.

Every route of include/sfk.h's SFK_IGEMM_ROUTES / SFK_WGRAD_ROUTES (the kernel instantiations reachable with the default
tuning table) gets the smallest shape that reaches it, already ragged -- a last tile of one row, an output-channel count
that is no multiple of the tile, a K tail, maps that are channel slices of wider pixel records at base addresses that are
16-byte but not 256-byte aligned -- plus the edges particular to it.  A case binds ONE call through a launch_audit.Recorder
(binding launches nothing) and DECLARES the route it is meant to reach; the tests compare that with what the library
reports (sfk_conv_igemm_route / sfk_conv_wgrad_route: the launch code run dry), so a retune that moves a shape to another
kernel fails instead of silently covering less.  The values come from launch_audit.replay's seeded fill, the verdict from
ref64.compare."""
from __future__ import annotations

import dataclasses
import functools
import os
import re
from typing import Callable, Dict, List, Optional, Tuple

import torch

from emu_backend import EmuBackend, _tile_bm
from video_classification_amd import plan
from video_classification_amd._lib import BnBwdFuse, ConvEpilogue, ConvPass, FMap, WgradPass

BF16, F32 = torch.bfloat16, torch.float32
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfk.h")
IK = {"REG": 0, "DMA": 1, "PWP": 2, "PWF": 3, "P8": 4, "HALO": 5, "PWD": 6}
WK = {"CFG": 0, "DMA": 1, "P8": 2, "BAND": 3}
FAMILY_OF_KERNEL = {0: 0, 1: 1, 2: 3, 3: 3, 4: 4, 5: 5, 6: 3}


def IR(kernel, bf16, bm, bn, epi=0, shortk=0, wide=0) -> int:
    """SFK_IGEMM_ROUTE of include/sfk.h"""
    return (bf16 << 28) | (IK[kernel] << 24) | (bm << 15) | (bn << 5) | (epi << 2) | (shortk << 1) | wide


def WR(kernel, bf16, tco, tci, ksnw, gram=0, dg=0) -> int:
    """SFK_WGRAD_ROUTE of include/sfk.h"""
    return (bf16 << 28) | (WK[kernel] << 24) | (tco << 15) | (tci << 6) | (ksnw << 2) | (gram << 1) | dg


@functools.lru_cache(maxsize=None)
def header_routes() -> Tuple[Dict[int, str], Dict[int, str]]:
    """the two route lists as include/sfk.h declares them: value -> name"""
    text = open(_HDR).read()

    def block(macro):
        body = text[text.index(f"#define {macro}(X)"):]
        lines = []
        for ln in body.split("\n")[1:]:
            lines.append(ln)
            if not ln.rstrip().endswith("\\"):
                break
        return re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", "\n".join(lines))
    ig = {IR(k, *map(int, r)): f"{k}_T{r[0]}_{r[1]}x{r[2]}_E{r[3]}_S{r[4]}_W{r[5]}" for k, *r in block("SFK_IGEMM_ROUTES")}
    wg = {WR(k, *map(int, r)): f"{k}_T{r[0]}_{r[1]}x{r[2]}_N{r[3]}_G{r[4]}_D{r[5]}" for k, *r in block("SFK_WGRAD_ROUTES")}
    return ig, wg


def route_name(r: int) -> str:
    ig, wg = header_routes()
    return ig.get(r) or wg.get(r) or hex(r)


# ----------------------------------------------------------------------------- the reference backend of the table
class EdgeEmu(EmuBackend):
    """EmuBackend plus the BatchNorm-backward reduce fused into a data-gradient pass with a conv output y_bn
    (sfk_bn_bwd_fuse flavours 1, 6, 7: include/sfk.h), which the CPU engine never binds"""

    def conv_igemm(self, p: ConvPass):
        if p.bnb is None or p.bnb.y_bn is None:
            return super().conv_igemm(p)
        b = p.bnb
        inner = super().conv_igemm(dataclasses.replace(p, bnb=None))

        def run(stream):
            inner(stream)                                      # dA, rounded once; the 0 / 1 mask keeps that rounding
            sl = tuple(slice(o, o + (r - 1) * s + 1, s) for o, s, r in zip(p.oo, p.os, p.rows))
            dest = p.y.view5()[:, sl[0], sl[1], sl[2]]
            yb = b.y_bn.view5().float()
            if b.mask_src is not None:
                m = b.mask_src.view5().float() > 0
            elif b.relu:
                m = yb * b.scale[: p.cout].float() + b.shift[: p.cout].float() > 0
            else:
                m = torch.ones_like(yb, dtype=torch.bool)
            dest.copy_((dest.float() * m).to(dest.dtype))
            dz = dest.float().reshape(-1, p.cout)
            xh = ((yb - b.mean[: p.cout].float()) * b.invstd[: p.cout].float()).reshape(-1, p.cout)
            bm = _tile_bm(p.cout)
            mt = (dz.shape[0] + bm - 1) // bm
            st = b.partials[: mt * p.cout * 2].view(mt, p.cout, 2)
            for i in range(mt):
                st[i, :, 0] = dz[i * bm:(i + 1) * bm].sum(0)
                st[i, :, 1] = (dz[i * bm:(i + 1) * bm] * xh[i * bm:(i + 1) * bm]).sum(0)
        return run


# ----------------------------------------------------------------------------- operands
def _buf(numel: int, dtype, device, mis: bool = True) -> torch.Tensor:
    """numel elements whose base address is 16 (mis) or 0 modulo 256"""
    es = torch.tensor([], dtype=dtype).element_size()
    raw = torch.zeros(numel * es + 512, dtype=torch.uint8, device=device)
    off = ((16 if mis else 0) - raw.data_ptr()) % 256
    return raw[off:off + numel * es].view(dtype)


def _map(n, dims, c, dtype, device, lay=(0, 0), mis=True) -> FMap:
    """a map whose pixel record is lay[0] channels wider than c, starting at channel lay[1]"""
    t, h, w = dims
    ld = c + lay[0]
    return FMap(_buf(n * t * h * w * ld, dtype, device, mis), n, t, h, w, c, ld, lay[1])


@dataclasses.dataclass
class Case:
    name: str
    method: str                      # conv_igemm | conv_wgrad | conv_pw_dual | a BatchNorm method of launch_audit.AUDITED
    route: Optional[int]             # the declared route (None: conv_pw_dual has none)
    bind: Callable                   # (recorder, device) -> the bound pass (or None)
    ws: Optional[bool] = None        # conv_wgrad: the workspace path is expected
    many_splits: Optional[bool] = None
    slow: bool = False               # float64 reference too slow on the CPU: geometry and route only there
    relu_mask: bool = False          # a ReLU mask is evaluated from values (ambiguous-sign share applies)
    seed: int = 0


CASES: List[Case] = []
# float64 on the CPU takes tens of seconds at the thresholds of these kernels (p8: K >= 1024 and M >= 16384; the 256 x 256
# tile: K >= 512, M >= 32768, 256 channels; wgrad p8: 64 K-tiles of 64 pixels per split): route and geometry only there
SLOW_ON_CPU = ("bf16_dma_t256_256_wide", "bf16_dma_t256_256_narrow", "wg_bf16_p8_ragged")


def conv(name, route, dt, n, dims, cin, cout, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), *, dgrad=None, xl=(0, 0), yl=(0, 0),
         acc=False, stats=False, ep=None, rl=(0, 0), bnb=None, bl=(0, 0), ml=None, obits=False, perm=False, mis=True, seed=0):
    """one sfk_conv_igemm call.  Forward: x has `dims`, the pass is plan.fwd_pass of Conv3d(cin, cout, k, s, p).  dgrad = i:
    pass i of plan.dgrad_passes of Conv3d(cout, cin, k, s, p) whose INPUT has `dims` -- the pass reads dY (cin channels
    here) and scatters into dX (cout channels here).  xl / yl / rl / bl: (extra channels of the pixel record, c_off) of x, y,
    ep.res, bnb.y_bn and bnb.mask_src (ml; default: as y_bn).  ep: names of the sfk_conv_epilogue fields to bind."""
    vec = 8 if dt == BF16 else 4

    def bind(rec, dev):
        if dgrad is None:
            g = plan.ConvGeom(cin, cout, k, s, p)
            ps = plan.fwd_pass(g, dims)
            xd, yd = dims, g.out_dims(dims)
        else:
            g = plan.ConvGeom(cout, cin, k, s, p)
            ps = plan.dgrad_passes(g, dims)[0][dgrad]
            xd, yd = g.out_dims(dims), dims
        taps = list(ps.taps)
        if perm:
            taps = taps[1::2] + taps[0::2]                    # widx no longer in tap order
        x, y = _map(n, xd, cin, dt, dev, xl, mis), _map(n, yd, cout, dt, dev, yl, mis)
        w = _buf(cout * g.wtaps * cin, dt, dev, mis)
        q = ConvPass(x, y, ps.rows, ps.gs, ps.os, ps.oo, taps, w, g.wtaps, cin, cout, accumulate=acc)
        f = lambda: _buf(cout, F32, dev, False)               # noqa: E731
        if obits:
            q.relu_out_bits = _buf(y.pixels * (cout // vec), torch.uint8, dev, False)
        if ep:
            e = ConvEpilogue()
            for fld in ep:
                if fld == "res":
                    e.res = _map(n, yd, cout, dt, dev, rl, mis)
                elif fld == "relu":
                    e.relu = True
                elif fld == "relu_bits":
                    e.relu_bits = _buf(y.pixels * (cout // vec), torch.uint8, dev, False)
                else:
                    setattr(e, fld, f())
            q.ep = e
        if bnb:
            b = BnBwdFuse(None, None, None, None, None, None, False, _buf(2 * cout, F32, dev, False))
            if bnb != 5:
                b.y_bn = _map(n, yd, cout, dt, dev, bl, mis)
                b.mean, b.invstd = f(), f()
                if bnb == 7:
                    b.mask_src = _map(n, yd, cout, dt, dev, bl if ml is None else ml, mis)
                else:
                    b.relu, b.scale, b.shift = True, f(), f()
            q.bnb = b
            b.partials = _buf((rec.conv_igemm_mtiles(q) + 2) * cout * 2, F32, dev, False)
        if stats:
            q.stats = _buf((rec.conv_igemm_mtiles(q) + 2) * cout * 2, F32, dev, False)
        rec.conv_igemm(q)
        return q
    CASES.append(Case(name, "conv_igemm", route, bind, slow=name in SLOW_ON_CPU, relu_mask=bnb in (1, 6), seed=seed))


def wgrad(name, route, dt, n, dims, cin, cout, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), *, ws="full", many=None, xl=(0, 0),
          dl=(0, 0), subset=None, gram=False, dg=None, mis=True, seed=0, expect_ws=None):
    """one sfk_conv_wgrad call of Conv3d(cin, cout, k, s, p) over an input of `dims`.  ws: "full" (the bytes the library asks
    for), "small" (16 bytes less: must fall back to atomics) or None.  subset: indices of the taps to list (the others
    must keep their dw).  gram: dy IS x.  dg: (extra channels, c_off) of the fused data gradient's output."""
    def bind(rec, dev):
        g = plan.ConvGeom(cin, cout, k, s, p)
        taps = list(plan.wgrad_taps(g))
        if subset is not None:
            taps = [taps[i] for i in subset]
        x = _map(n, dims, cin, dt, dev, xl, mis)
        dy = x if gram else _map(n, g.out_dims(dims), cout, dt, dev, dl, mis)
        q = WgradPass(x, dy, g.s, taps, _buf(cout * g.wtaps * cin, F32, dev, False), g.wtaps, cin, cout)
        if dg is not None:
            q.dg_w = _buf(cin * cout, dt, dev, False)
            q.dg_y = _map(n, dims, cin, dt, dev, dg, mis)
        if ws is not None:
            nbytes = rec.conv_wgrad_workspace_bytes(q) - (16 if ws == "small" else 0)
            if nbytes > 0:
                q.workspace = _buf(nbytes // 4, F32, dev, False)
        rec.conv_wgrad(q)
        return q
    CASES.append(Case(name, "conv_wgrad", route, bind, ws=(ws == "full") if expect_ws is None else expect_ws, many_splits=many, slow=name in SLOW_ON_CPU,
                      seed=seed))


def pw_dual(name, c1, c2, co, px, l1=(0, 0), l2=(0, 0), ly=(0, 0), bias=True):
    def bind(rec, dev):
        x1, x2 = _map(1, (1, 1, px), c1, BF16, dev, l1), _map(1, (1, 1, px), c2, BF16, dev, l2)
        y = _map(1, (1, 1, px), co, BF16, dev, ly)
        rec.conv_pw_dual(x1, _buf(co * c1, BF16, dev), x2, _buf(co * c2, BF16, dev), _buf(co, F32, dev, False) if bias else None, y)
        return None
    CASES.append(Case(name, "conv_pw_dual", None, bind))


def PW(m):
    return (1, 1, m)


# ============================================================================= sfk_conv_igemm: register-staged, f32
S3 = dict(k=(1, 3, 3), p=(0, 1, 1))
K27 = dict(k=(3, 3, 3), p=(1, 1, 1))
conv("f32_reg128_last_row", IR("REG", 0, 128, 128), F32, 1, PW(129), 4, 132, xl=(8, 4), yl=(8, 4))       # K tail of 4
conv("f32_reg128_one_pixel_stats", IR("REG", 0, 128, 128), F32, 1, PW(1), 80, 132, stats=True)
conv("f32_reg64_stride2_pad", IR("REG", 0, 256, 64), F32, 1, (1, 33, 31), 40, 36, **S3, s=(1, 2, 2), xl=(4, 4), yl=(4, 0),
     stats=True)
conv("f32_reg64_dgrad_s2_pass0", IR("REG", 0, 256, 64), F32, 1, (2, 17, 15), 40, 36, **K27, s=(1, 2, 2), dgrad=0, yl=(4, 4))
conv("f32_reg64_dgrad_s2_pass1", IR("REG", 0, 256, 64), F32, 1, (2, 17, 15), 40, 36, **K27, s=(1, 2, 2), dgrad=1, acc=True)
conv("f32_reg64_dgrad_s2_pass2", IR("REG", 0, 256, 64), F32, 1, (2, 17, 15), 40, 36, **K27, s=(1, 2, 2), dgrad=2, acc=True)
conv("f32_reg64_dgrad_s2_pass3", IR("REG", 0, 256, 64), F32, 1, (2, 17, 15), 40, 36, **K27, s=(1, 2, 2), dgrad=3, acc=True,
     yl=(8, 4))
conv("f32_reg32_long_k", IR("REG", 0, 256, 32), F32, 1, (3, 9, 9), 24, 20, **S3, perm=True)
conv("f32_reg32_short_k5", IR("REG", 0, 256, 32, 0, 1), F32, 1, PW(257), 160, 24, xl=(4, 4))              # KC = 5
conv("f32_reg32_k6", IR("REG", 0, 256, 32), F32, 1, PW(255), 164, 24, acc=True)                            # KC = 6
conv("f32_reg16_long_k_acc", IR("REG", 0, 256, 16), F32, 1, (3, 8, 8), 24, 8, **S3, acc=True, yl=(4, 4))
conv("f32_reg16_short_one_pixel", IR("REG", 0, 256, 16, 0, 1), F32, 1, PW(1), 80, 16)
conv("f32_reg16_short_4ch", IR("REG", 0, 256, 16, 0, 1), F32, 1, PW(255), 4, 4, xl=(4, 0), yl=(4, 4), stats=True)
conv("f32_reg16_lateral_7", IR("REG", 0, 256, 16, 0, 1), F32, 1, (29, 3, 3), 8, 16, k=(7, 1, 1), s=(4, 1, 1), p=(3, 0, 0))
conv("f32_reg128_bits", IR("REG", 0, 128, 128, 2), F32, 1, PW(129), 8, 132, obits=True, yl=(4, 4))
conv("f32_reg64_bits_acc", IR("REG", 0, 256, 64, 2), F32, 1, PW(257), 40, 36, obits=True, acc=True)
conv("f32_reg32_bits", IR("REG", 0, 256, 32, 2), F32, 1, PW(255), 8, 20, obits=True)
conv("f32_reg16_bits", IR("REG", 0, 256, 16, 2), F32, 1, PW(257), 4, 8, obits=True)
conv("f32_reg128_ep_all", IR("REG", 0, 128, 128, 3), F32, 1, PW(129), 40, 132,
     ep=("scale", "shift", "res", "res_scale", "res_shift", "relu", "relu_bits"), rl=(8, 4), yl=(4, 4))
conv("f32_reg64_ep_res_acc", IR("REG", 0, 256, 64, 3), F32, 1, PW(257), 8, 64, ep=("scale", "res"), acc=True, rl=(4, 0))
conv("f32_reg32_ep_shift_acc", IR("REG", 0, 256, 32, 3), F32, 1, (1, 9, 9), 8, 20, **S3, ep=("shift",), acc=True)
conv("f32_reg16_ep_relu", IR("REG", 0, 256, 16, 3), F32, 1, PW(255), 8, 12, ep=("scale", "relu", "relu_bits"))

# ============================================================================= register-staged, bf16 (cout <= 64)
conv("bf16_reg64_wide_stride2", IR("REG", 1, 256, 64, 0, 0, 1), BF16, 1, (1, 33, 31), 80, 64, **S3, s=(1, 2, 2), xl=(8, 8),
     yl=(8, 8), stats=True)
conv("bf16_reg64_narrow_coff4", IR("REG", 1, 256, 64, 0, 0, 0), BF16, 1, PW(257), 40, 40, yl=(8, 4), stats=True)
conv("bf16_reg64_narrow_cout36", IR("REG", 1, 256, 64, 0, 0, 0), BF16, 1, PW(255), 8, 36, acc=True)
conv("bf16_reg64_more_tiles_than_resident", IR("REG", 1, 256, 64, 0, 0, 1), BF16, 1, PW(256 * 800 + 1), 8, 40, xl=(8, 0))
conv("bf16_reg32_long_wide", IR("REG", 1, 256, 32, 0, 0, 1), BF16, 1, (3, 9, 9), 24, 24, **S3, perm=True)
conv("bf16_reg32_long_narrow", IR("REG", 1, 256, 32, 0, 0, 0), BF16, 1, (3, 9, 9), 24, 20, **S3, acc=True)
conv("bf16_reg32_short_wide", IR("REG", 1, 256, 32, 0, 1, 1), BF16, 1, PW(257), 40, 32, xl=(8, 8), yl=(8, 8), stats=True)
conv("bf16_reg32_short_narrow_k5", IR("REG", 1, 256, 32, 0, 1, 0), BF16, 1, PW(255), 160, 28)
conv("bf16_reg32_k6_narrow", IR("REG", 1, 256, 32, 0, 0, 0), BF16, 1, PW(257), 168, 24, yl=(8, 4))
conv("bf16_reg16_long_half_fragment", IR("REG", 1, 256, 16, 0, 0, 0), BF16, 1, (3, 8, 8), 24, 8, **S3, stats=True)
conv("bf16_reg16_short_one_pixel", IR("REG", 1, 256, 16, 0, 1, 0), BF16, 1, PW(1), 8, 16)
conv("bf16_reg16_short_12ch_acc", IR("REG", 1, 256, 16, 0, 1, 0), BF16, 1, PW(257), 80, 12, acc=True, yl=(4, 4))
conv("bf16_reg16_lateral_4", IR("REG", 1, 256, 16, 0, 1, 0), BF16, 1, (30, 3, 3), 8, 16, k=(4, 1, 1), s=(4, 1, 1), p=(0, 0, 0))
conv("bf16_reg64_ep_res_relu", IR("REG", 1, 256, 64, 3, 0, 1), BF16, 1, (1, 9, 13), 16, 64, **S3,
     ep=("scale", "shift", "res", "res_scale", "res_shift", "relu", "relu_bits"), rl=(8, 8), yl=(8, 8))
conv("bf16_reg32_ep_res_acc", IR("REG", 1, 256, 32, 3, 0, 1), BF16, 1, PW(257), 40, 24, ep=("shift", "res", "res_shift"),
     acc=True)
conv("bf16_reg16_ep_scale_shift_acc", IR("REG", 1, 256, 16, 3, 0, 0), BF16, 1, PW(255), 8, 16, ep=("scale", "shift"), acc=True)
for _bn, _co in ((64, 64), (32, 24)):
    conv(f"bf16_reg{_bn}_bits", IR("REG", 1, 256, _bn, 2, 0, 1), BF16, 1, PW(257), 16, _co, obits=True, yl=(8, 8))
    conv(f"bf16_reg{_bn}_bnb1", IR("REG", 1, 256, _bn, 1, 0, 1), BF16, 1, PW(257), 16, _co, bnb=1, bl=(8, 8))
    conv(f"bf16_reg{_bn}_bnb5", IR("REG", 1, 256, _bn, 5, 0, 1), BF16, 1, PW(255), 16, _co, bnb=5, obits=True, acc=True)
    conv(f"bf16_reg{_bn}_bnb6", IR("REG", 1, 256, _bn, 6, 0, 1), BF16, 1, PW(513), 40, _co, bnb=6, acc=True, yl=(8, 8))
    conv(f"bf16_reg{_bn}_bnb7", IR("REG", 1, 256, _bn, 7, 0, 1), BF16, 1, (1, 9, 9), 8, _co, **S3, bnb=7, bl=(8, 0))
    # y, y_bn and mask_src each with a layout of its own: a swapped ld / c_off pair reads another map's channels
    conv(f"bf16_reg{_bn}_bnb7_sliced", IR("REG", 1, 256, _bn, 7, 0, 1), BF16, 1, PW(257), 40, _co, bnb=7, bl=(8, 8), ml=(24, 16),
         yl=(16, 8), acc=True)

# ============================================================================= LDS-DMA ring (bf16, cout > 64)
conv("bf16_dma128_wide_last_row", IR("DMA", 1, 128, 128, 0, 0, 1), BF16, 1, PW(257), 80, 136, xl=(8, 8), yl=(8, 8), stats=True)
conv("bf16_dma128_narrow_cout132", IR("DMA", 1, 128, 128, 0, 0, 0), BF16, 1, PW(127), 8, 132, acc=True)
conv("bf16_dma128_narrow_coff4", IR("DMA", 1, 128, 128, 0, 0, 0), BF16, 1, (1, 9, 9), 40, 136, **S3, yl=(8, 4), stats=True)
conv("bf16_dma128_one_pixel", IR("DMA", 1, 128, 128, 0, 0, 1), BF16, 1, PW(1), 40, 136)
conv("bf16_dma128_dgrad_s2_pass0", IR("DMA", 1, 128, 128, 0, 0, 1), BF16, 1, (2, 17, 15), 40, 136, **K27, s=(1, 2, 2), dgrad=0)
conv("bf16_dma128_dgrad_s2_pass3", IR("DMA", 1, 128, 128, 0, 0, 1), BF16, 1, (2, 17, 15), 40, 136, **K27, s=(1, 2, 2), dgrad=3,
     acc=True, yl=(8, 8))
conv("bf16_dma256x128_wide", IR("DMA", 1, 256, 128, 0, 0, 1), BF16, 1, PW(32769), 8, 136, yl=(8, 8))
conv("bf16_dma256x128_narrow", IR("DMA", 1, 256, 128, 0, 0, 0), BF16, 1, PW(32769), 40, 132, acc=True)
conv("bf16_dma_t256_224_wide", IR("DMA", 1, 224, 256, 0, 0, 1), BF16, 1, PW(32769), 512, 256)
conv("bf16_dma_t256_224_narrow", IR("DMA", 1, 224, 256, 0, 0, 0), BF16, 1, PW(32769), 520, 256, yl=(8, 4))
conv("bf16_dma_t256_256_wide", IR("DMA", 1, 256, 256, 0, 0, 1), BF16, 1, PW(57601), 512, 256, acc=True)
conv("bf16_dma_t256_256_narrow", IR("DMA", 1, 256, 256, 0, 0, 0), BF16, 1, PW(57601), 512, 256, yl=(8, 4))
conv("bf16_dma128_bnb1", IR("DMA", 1, 128, 128, 1, 0, 1), BF16, 1, PW(257), 16, 136, bnb=1, bl=(8, 8), yl=(8, 8))
conv("bf16_dma128_bnb5", IR("DMA", 1, 128, 128, 5, 0, 1), BF16, 1, PW(127), 40, 136, bnb=5, obits=True)
conv("bf16_dma128_bnb6", IR("DMA", 1, 128, 128, 6, 0, 1), BF16, 1, PW(257), 80, 136, bnb=6, acc=True)
conv("bf16_dma128_bnb7", IR("DMA", 1, 128, 128, 7, 0, 1), BF16, 1, (1, 9, 9), 8, 136, **S3, bnb=7, bl=(8, 0))
conv("bf16_dma128_bnb7_sliced", IR("DMA", 1, 128, 128, 7, 0, 1), BF16, 1, PW(257), 40, 136, bnb=7, bl=(8, 8), ml=(24, 16),
     yl=(16, 8))
conv("bf16_dma128_bnb7_sliced_acc", IR("DMA", 1, 128, 128, 7, 0, 1), BF16, 1, PW(127), 16, 136, bnb=7, bl=(16, 8), ml=(8, 8), acc=True)
conv("bf16_dma128_bits", IR("DMA", 1, 128, 128, 2, 0, 1), BF16, 1, PW(257), 40, 136, obits=True, acc=True)
conv("bf16_dma256x128_bits", IR("DMA", 1, 256, 128, 2, 0, 1), BF16, 1, PW(32769), 8, 136, obits=True)
conv("bf16_dma128_ep_shift", IR("DMA", 1, 128, 128, 3, 0, 1), BF16, 1, PW(257), 40, 136, ep=("shift",), acc=True, yl=(8, 8))
conv("bf16_dma256x128_ep_relu", IR("DMA", 1, 256, 128, 3, 0, 1), BF16, 1, PW(32769), 8, 136,
     ep=("scale", "shift", "relu", "relu_bits"))
conv("bf16_dma128_ep_res", IR("DMA", 1, 128, 128, 4, 0, 1), BF16, 1, PW(257), 40, 136,
     ep=("scale", "res", "res_scale", "res_shift", "relu", "relu_bits"), rl=(8, 8), yl=(8, 8))

# ============================================================================= deep-pipelined 256 x 256 tile, LDS band
conv("bf16_p8_256", IR("P8", 1, 256, 256, 0, 0, 1), BF16, 1, PW(16385), 1024, 256, yl=(8, 8))
conv("bf16_p8_256_bits_acc", IR("P8", 1, 256, 256, 2, 0, 1), BF16, 1, PW(16385), 1024, 256, obits=True, acc=True)
conv("bf16_halo_one_band", IR("HALO", 1, 224, 64, 0, 0, 1), BF16, 1, (1, 4, 56), 64, 64, **S3, xl=(8, 8), yl=(8, 8), stats=True)
conv("bf16_halo_258_bands_perm", IR("HALO", 1, 224, 64, 0, 0, 1), BF16, 1, (129, 8, 56), 64, 64, **S3, perm=True, stats=True)

# ============================================================================= streaming pointwise kernels
_EPS = {32: ("scale", "res", "relu", "relu_bits"), 64: ("shift", "res", "res_scale", "res_shift"),
        128: ("scale", "shift", "relu"), 256: ("scale", "shift", "res", "res_scale", "res_shift", "relu", "relu_bits"),
        320: ("scale", "relu", "relu_bits"), 512: ("shift", "res", "res_shift", "relu")}
for _co, _k, _ci in ((32, 32, 8), (64, 32, 24), (64, 64, 40), (128, 32, 32), (128, 128, 104), (256, 64, 40), (320, 128, 104),
                     (512, 128, 128)):
    conv(f"bf16_pw_fused_{_ci}_{_co}", IR("PWF", 1, _k, _co, 0, 0, 1), BF16, 1, PW(777), _ci, _co, ep=_EPS[_co], xl=(8, 8),
         yl=(8, 8), rl=(8, 0))
conv("bf16_pw_fused_one_pixel", IR("PWF", 1, 64, 256, 0, 0, 1), BF16, 1, PW(1), 64, 256, ep=("scale", "res", "relu"))
conv("bf16_pw_plain_64_acc", IR("PWP", 1, 64, 64, 0, 0, 1), BF16, 1, PW(777), 64, 64, acc=True, yl=(8, 8))
conv("bf16_pw_plain_128_bias_acc", IR("PWP", 1, 128, 128, 0, 0, 1), BF16, 1, PW(777), 128, 128, acc=True, ep=("shift",), xl=(8, 8))
conv("bf16_pw_plain_320", IR("PWP", 1, 128, 320, 0, 0, 1), BF16, 1, PW(777), 128, 320, yl=(8, 8))
conv("bf16_pw_dgrad_64_256", IR("PWD", 1, 64, 256, 1, 0, 1), BF16, 1, PW(777), 64, 256, acc=True, obits=True, bnb=5, yl=(8, 8))
conv("bf16_pw_dgrad_128_512", IR("PWD", 1, 128, 512, 1, 0, 1), BF16, 1, PW(777), 128, 512, acc=True, obits=True, bnb=5, xl=(8, 8))
pw_dual("bf16_pw_dual_8_ragged", 32, 8, 8, 777, l1=(8, 8), ly=(8, 8))
pw_dual("bf16_pw_dual_16_one_pixel", 64, 16, 16, 1, l2=(8, 0), bias=False)
pw_dual("bf16_pw_dual_16_ragged", 64, 16, 16, 4097, ly=(16, 8))

# ============================================================================= sfk_conv_wgrad
T3 = dict(k=(3, 1, 1), p=(1, 0, 0))
for _b, _dt, _v in ((0, F32, 4), (1, BF16, 8)):
    _t = "bf16" if _b else "f32"
    wgrad(f"wg_{_t}_32x32_one_pixel", WR("CFG", _b, 32, 32, 4), _dt, 1, (1, 1, 1), _v, 24, **T3, many=False)
    wgrad(f"wg_{_t}_32x32_m63_subset", WR("CFG", _b, 32, 32, 4), _dt, 1, (7, 3, 3), _v, 24, **T3, subset=(2, 0), xl=(_v, _v),
          ws=None)
    wgrad(f"wg_{_t}_64x32_m65", WR("CFG", _b, 64, 32, 4), _dt, 1, (1, 5, 13), 3 * _v, 40, ws="small", dl=(_v, _v))
    wgrad(f"wg_{_t}_128x32_many", WR("CFG", _b, 128, 32, 2), _dt, 1, (1, 1, 64 * 64 + 1), _v, 72, many=True)
    wgrad(f"wg_{_t}_32x128_stride2", WR("CFG", _b, 32, 128, 2), _dt, 1, (1, 17, 15), 40, 24, **S3, s=(1, 2, 2), ws=None)
    wgrad(f"wg_{_t}_64x128_9taps", WR("CFG", _b, 64, 128, 2), _dt, 1, (1, 9, 7), 2 * _v, 40, **S3, subset=(0, 2, 4, 5, 8), many=False)
    wgrad(f"wg_{_t}_128x128_m65", WR("CFG", _b, 128, 128, 1), _dt, 1, PW(65), 40, 136, xl=(_v, 0), dl=(_v, _v))
    wgrad(f"wg_{_t}_gram32", WR("CFG", _b, 32, 32, 4, 1), _dt, 1, PW(129), 24, 24, gram=True, xl=(_v, _v))
    wgrad(f"wg_{_t}_gram64", WR("CFG", _b, 64, 64, 2, 1), _dt, 1, PW(63), 40, 40, gram=True, ws=None)
    wgrad(f"wg_{_t}_gram128", WR("CFG", _b, 128, 128, 1, 1), _dt, 1, PW(4097), 72, 72, gram=True, many=True)
wgrad("wg_bf16_256x64_ragged", WR("CFG", 1, 256, 64, 1), BF16, 1, PW(65), 40, 264, dl=(8, 8))
wgrad("wg_bf16_dma128_ws", WR("DMA", 1, 128, 128, 4), BF16, 1, PW(65), 136, 136, xl=(8, 8))
wgrad("wg_bf16_dma128_small_ws", WR("DMA", 1, 128, 128, 4), BF16, 1, PW(2049), 136, 136, ws="small", many=True)
wgrad("wg_bf16_dma128_atomics_taps", WR("DMA", 1, 128, 128, 4), BF16, 1, (1, 9, 7), 40, 136, **S3, subset=(1, 3, 4, 7), ws=None)
wgrad("wg_bf16_dma128_one_pixel", WR("DMA", 1, 128, 128, 4), BF16, 1, PW(1), 128, 128)
wgrad("wg_bf16_dma256_cols64", WR("DMA", 1, 256, 128, 8), BF16, 1, PW(2049), 64, 256, many=True)
wgrad("wg_bf16_dma256_cols64_atomics", WR("DMA", 1, 256, 128, 8), BF16, 1, PW(63), 64, 256, ws=None)
wgrad("wg_bf16_dma256_big", WR("DMA", 1, 256, 128, 8), BF16, 1, PW(123393), 136, 264, many=True)
wgrad("wg_bf16_dma256_dg_slice", WR("DMA", 1, 256, 128, 8, 0, 1), BF16, 1, PW(65), 64, 256, dg=(8, 8))
wgrad("wg_bf16_dma256_dg_many", WR("DMA", 1, 256, 128, 8, 0, 1), BF16, 1, PW(4097), 64, 256, dg=(0, 0), ws=None, many=True)
wgrad("wg_bf16_p8_ragged", WR("P8", 1, 256, 256, 8), BF16, 1, PW(65537), 512, 512, many=True)
wgrad("wg_bf16_band56_65_bands", WR("BAND", 1, 64, 64, 8), BF16, 5, (13, 4, 56), 64, 64, **S3, many=True)
wgrad("wg_bf16_band28_65_bands", WR("BAND", 1, 128, 128, 8), BF16, 5, (13, 4, 28), 128, 128, **S3, many=True, xl=(8, 8))
wgrad("wg_bf16_band56_small_ws_falls_back", WR("CFG", 1, 64, 128, 2), BF16, 5, (13, 4, 56), 64, 64, **S3, ws="small", many=True,
      expect_ws=True)     # too small for the band kernel's partials, enough for the register-staged tile's


# ============================================================================= BatchNorm reductions and the stem tail at small shapes
# (already restated by launch_audit; here at the channel-group counts 1, 10, 256 and 288 -- one lane, a partial wave, one
# chunk of 256 groups, a partial second chunk --, at 1 pixel, one block of pixel rows minus 1 and one span of blocks plus 1,
# with max_parts 1 / 3 / 1024, and the stem tail over frames of 1 x 1 .. 7 x 5)
def bn(name, method, dt, c, n, dims, mp=0, flavour=0, lay=(0, 0)):
    vec = 8 if dt == BF16 else 4

    def bind(rec, dev):
        f = lambda: _buf(c, F32, dev, False)                  # noqa: E731
        y = _map(n, dims, c, dt, dev, lay)
        parts = _buf(max(mp, 1) * c * 2, F32, dev, False)              # (1024 rows of 288 groups in bf16: 18.9 MB)
        if method == "bn_stats":
            rec.bn_stats(y, parts, mp)
        elif method == "bn_bwd_reduce":
            da = _map(n, dims, c, dt, dev, lay)
            if flavour == 0:                                  # mask from the values, no dz
                rec.bn_bwd_reduce(da, y, None, f(), f(), f(), f(), True, None, parts, mp)
            elif flavour == 1:                                # mask from the bitmap, dz written
                rec.bn_bwd_reduce(da, y, None, f(), f(), None, None, False, _map(n, dims, c, dt, dev, lay), parts, mp,
                                  _buf(y.pixels * (c // vec), torch.uint8, dev, False))
            else:                                             # mask source, dz in place
                rec.bn_bwd_reduce(da, y, _map(n, dims, c, dt, dev), f(), f(), None, None, False, da, parts, mp)
        else:
            od = (dims[0], (dims[1] - 1) // 2 + 1, (dims[2] - 1) // 2 + 1)
            out = _map(n, od, c, dt, dev, lay)
            arg = _buf(out.pixels * c, torch.uint8, dev, False)
            if method == "bn_maxpool_fwd":
                rec.bn_maxpool_fwd(y, f(), f(), out, arg, 3, 2, 1)
            elif method == "bn_maxpool_bwd_reduce":
                rec.bn_maxpool_bwd_reduce(out, arg, y, f(), f(), f(), f(), parts, mp)
            else:
                rec.bn_maxpool_bwd_apply(out, arg, y, f(), f(), f(), f(), _buf(c * 3, F32, dev, False), _map(n, dims, c, dt, dev, lay))
        return None
    CASES.append(Case(name, method, None, bind, relu_mask=method != "bn_stats" and flavour == 0))


for _dt, _t, _v in ((BF16, "bf16", 8), (F32, "f32", 4)):
    for _gi, _g in enumerate((1, 10, 256, 288)):
        _rb = 256 // min(_g, 256)                             # pixel rows of a 256-thread block (csrc/bn.hip)
        for _pi, _px in enumerate(sorted({1, max(_rb - 1, 2), 4 * _rb + 1})):
            _mp = (1, 3, 1024)[(_gi + _pi) % 3]
            _lay = (_v, _v) if (_gi + _pi) % 2 else (0, 0)
            bn(f"bn_stats_{_t}_g{_g}_px{_px}_mp{_mp}", "bn_stats", _dt, _g * _v, 1, (1, 1, _px), _mp, lay=_lay)
            bn(f"bn_bwd_reduce_{_t}_g{_g}_px{_px}_mp{_mp}", "bn_bwd_reduce", _dt, _g * _v, 1, (1, 1, _px), _mp, flavour=_pi % 3,
               lay=_lay)
    for _fi, (_h, _w) in enumerate(((1, 1), (2, 3), (7, 5))):
        for _g in (1, 10, 256, 288):
            _mp = (1, 3, 1024)[_fi]
            bn(f"bn_maxpool_fwd_{_t}_g{_g}_{_h}x{_w}", "bn_maxpool_fwd", _dt, _g * _v, 2, (3, _h, _w), lay=(_v, 0) if _fi else (0, 0))
            bn(f"bn_maxpool_bwd_reduce_{_t}_g{_g}_{_h}x{_w}", "bn_maxpool_bwd_reduce", _dt, _g * _v, 2, (3, _h, _w), _mp)
            bn(f"bn_maxpool_bwd_apply_{_t}_g{_g}_{_h}x{_w}", "bn_maxpool_bwd_apply", _dt, _g * _v, 2, (3, _h, _w), lay=(_v, _v))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
