"""TEST INFRASTRUCTURE: the case table of the stem edge audit (tests/test_stem_edges_cpu.py, tests/test_gpu_stem_edges.py).
No GPU import.

Every route of include/sfk.h's SFK_STEM_ROUTES (the stem kernel instantiations reachable with the default tuning table) gets
the smallest shapes that reach it, ragged from the start: half tiles of 8 rows below, across and beyond their edge, tile
columns of 4 and a partial second tile, temporal pairs with a trailing half pair and one, two and three pair chunks, frame
tables that repeat and go backwards, sources that are channel slices of N,T,C,H,W memory, more units than workgroups.  Every
map is a channel slice (ld > c, c_off > 0) of a wider pixel record, every base pointer sits at 16 modulo 256, dw starts
non-zero and `stats` carries two poisoned rows past the tile count.  A case binds ONE call through a launch_audit.Recorder
(binding launches nothing) and DECLARES its route -- or the sfk_status with which the call must be refused, nothing written
--; the tests compare that with sfk_stem_conv_fwd_route / sfk_stem_conv_wgrad_route (the launch code run dry).  Values come
from launch_audit.replay's seeded fill, the verdict from ref64.compare against launch_audit's float64 restatements.

The uint8 and pooled stems cannot be recorded (their source is no tensor): `u8_run` holds them to the same restatement on
the materialised clip (tests/emu_u8stem.py, tests/emu_u8stem_pool.py state the header's formula), with the same guard and
untouched-byte checks, and the GPU test adds bit-identity to the float entry point on that clip."""
from __future__ import annotations

import dataclasses
import functools
import os
import re
from typing import Callable, Dict, List, Optional, Tuple

import torch

import launch_audit as la
import ref64
from conv_edges import _buf, _map
from video_classification_amd._lib import FMap, SfkError, StemSrc, stem_kp
from video_classification_amd.input_pipeline import PoolClip, U8Clip, normalize_lut

BF16, F32 = torch.bfloat16, torch.float32
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfk.h")
SK = {"V4": 0, "V2": 1, "S4": 2, "GENERIC": 3, "WGV2": 4, "WG_GENERIC": 5}
INVALID, UNSUPPORTED = -1, -2


def SR(kernel: str, map_bf16: int, src_bf16: int, n: int) -> int:
    """SFK_STEM_ROUTE of include/sfk.h"""
    return (SK[kernel] << 8) | (map_bf16 << 5) | (src_bf16 << 4) | n


@functools.lru_cache(maxsize=None)
def header_routes() -> Dict[int, str]:
    """SFK_STEM_ROUTES as include/sfk.h declares it: value -> name"""
    text = open(_HDR).read()
    body = text[text.index("#define SFK_STEM_ROUTES(X)"):]
    lines = []
    for ln in body.split("\n")[1:]:
        lines.append(ln)
        if not ln.rstrip().endswith("\\"):
            break
    rows = re.findall(r"X\((\w+), (\d+), (\d+), (\d+)\)", "\n".join(lines))
    return {SR(k, int(m), int(s), int(n)): f"{k}_M{m}_S{s}_N{n}" for k, m, s, n in rows}


def route_name(r: Optional[int]) -> str:
    return "none" if r is None else header_routes().get(r, hex(r))


def is_wgrad(method: str) -> bool:
    return method.endswith("wgrad")


# ----------------------------------------------------------------------------- operands
def _src(dev, dt, n, cin, t, h, w, mem="nc"):
    """the clip, indexed (n, c, t, h, w), its first element at 16 modulo 256.  mem: "nc" dense N,C,T,H,W; ("ntc", C, c0):
    channels c0 .. c0 + cin of dataset memory N,T,C,H,W; "w2": every second column of a frame twice as wide (sw = 2)"""
    if mem == "nc":
        return _buf(n * cin * t * h * w, dt, dev).view(n, cin, t, h, w)
    if mem == "w2":
        return _buf(n * cin * t * h * w * 2, dt, dev).view(n, cin, t, h, w * 2)[..., ::2]
    _, ctot, c0 = mem
    return _buf(n * t * ctot * h * w, dt, dev).view(n, t, ctot, h, w).permute(0, 2, 1, 3, 4)[:, c0:c0 + cin]


def _out(x: int) -> int:
    return (x - 1) // 2 + 1


@dataclasses.dataclass
class Case:
    name: str
    method: str                      # stem_conv_fwd | stem_conv_wgrad | stem2d_fwd | stem2d_wgrad
    route: Optional[int]             # the declared route (None: the 2-D stem has one instantiation per dtype pair, and no query)
    bind: Callable                   # (recorder, device) -> (StemSrc, map)
    status: int = 0                  # < 0: the call must be refused with this sfk_status and write nothing
    units: Optional[int] = None      # declared work items / workgroups (or blocks), where the case is about them
    grid: Optional[int] = None
    wrap: Optional[bool] = None      # more work items than workgroups
    twice: bool = False              # replay a second time (atomics: dw is held to float64 both times, the spread printed)
    seed: int = 0


CASES: List[Case] = []


def stem(name, route, mdt, sdt, n, cin, kt, t, h, w, cout, *, wg=False, ti=None, mem="nc", lay=(8, 8), status=0, units=None,
         grid=None, wrap=None, twice=False, mis=True, seed=0):
    """one sfk_stem_conv_fwd (or, wg, sfk_stem_conv_wgrad) call: a clip of n x cin x t x h x w in `sdt`, frames selected by
    ti, a (kt,7,7) filter with cout outputs, the map in `mdt` laid out as (extra channels of the pixel record, c_off)"""
    def bind(rec, dev):
        src = _src(dev, sdt, n, cin, t, h, w, mem)
        tix = None if ti is None else torch.tensor(ti, dtype=torch.int32, device=dev)
        p = StemSrc(src, tix, kt)
        m = _map(n, (p.t_len, _out(h), _out(w)), cout, mdt, dev, lay, mis)
        kp = stem_kp(cin, kt)
        if wg:
            rec.stem_conv_wgrad(p, m, _buf(cout * kp, F32, dev))
        else:
            rows = rec.stem_conv_tiles(p, m) + 2
            rec.stem_conv_fwd(p, _buf(cout * kp, mdt, dev), m, _buf(rows * cout * 2, F32, dev, False))
        return p, m
    CASES.append(Case(name, "stem_conv_wgrad" if wg else "stem_conv_fwd", route, bind, status, units, grid, wrap, twice, seed))


def stem2d(name, mdt, sdt, n, t, c, h, w, cout, *, wg=False, lay=(8, 8), status=0, seed=0):
    """one sfk_stem2d_fwd / _wgrad call: the frames-as-channels stem over T x C planes"""
    def bind(rec, dev):
        p = StemSrc(_src(dev, sdt, n, c, t, h, w), None, t)
        m = _map(n, (1, _out(h), _out(w)), cout, mdt, dev, lay)
        kp = stem_kp(c, t)
        if wg:
            rec.stem2d_wgrad(p, m, _buf(cout * kp, F32, dev))
        else:
            rows = n * ((_out(h) + 15) // 16) * ((_out(w) + 15) // 16) + 2
            rec.stem2d_fwd(p, _buf(cout * kp, mdt, dev), m, _buf(rows * cout * 2, F32, dev, False))
        return p, m
    CASES.append(Case(name, "stem2d_wgrad" if wg else "stem2d_fwd", None, bind, status, seed=seed))


# ============================================================================= V4: the fast stem's half-tile pair kernel
# units = clips x half tiles of 8 rows x tile columns x pair chunks (8 pairs, the last chunk takes the remainder and the half
# pair); h_in 2 / 13 / 17 / 33 -> ho 1 / 7 / 9 / 17, w_in 8 / 24 / 40 -> wo 4 / 12 / 20
V5, V3 = SR("V4", 1, 1, 5), SR("V4", 1, 1, 3)
stem("v4_k5_c8_t2_7x4", V5, BF16, BF16, 1, 3, 5, 2, 13, 8, 8, units=1, grid=1)
stem("v4_k5_c4_t3_1x12_coff4", V5, BF16, BF16, 2, 3, 5, 3, 2, 24, 4, lay=(12, 4), units=2)                # half pair; c_off % 8 == 4
stem("v4_k3_c8_t17_9x20", V3, BF16, BF16, 1, 3, 3, 17, 17, 40, 8, units=4, wrap=False)                     # nfull 8: one chunk of 9 pairs
stem("v4_k3_c4_t19_17x12", V3, BF16, BF16, 1, 3, 3, 19, 33, 24, 4, lay=(4, 4), units=6)                    # two chunks, the last with the half pair
stem("v4_k5_c8_t35_7x4", V5, BF16, BF16, 1, 3, 5, 35, 13, 8, 8, units=3)                                   # three chunks
stem("v4_k5_c8_t19_9x4", V5, BF16, BF16, 1, 3, 5, 19, 17, 8, 8, units=4)
stem("v4_k3_c8_t2_17x20", V3, BF16, BF16, 3, 3, 3, 2, 33, 40, 8, units=18, wrap=False)                     # below 512 and no multiple of 8: plain unit order
stem("v4_k5_c8_tindex_repeats", V5, BF16, BF16, 2, 3, 5, 6, 13, 24, 8, ti=(3, 1, 1, 5, 0))
stem("v4_k3_c4_tindex_long_clip", V3, BF16, BF16, 1, 3, 3, 64, 17, 8, 4, ti=(0, 9, 18, 27, 36, 45, 54, 63, 62), lay=(4, 4))
stem("v4_k5_c8_ntchw_slice", V5, BF16, BF16, 2, 3, 5, 3, 17, 24, 8, mem=("ntc", 8, 2))
stem("v4_k3_c8_ntchw_slice_tindex", V3, BF16, BF16, 2, 3, 3, 7, 13, 8, 8, mem=("ntc", 5, 1), ti=(6, 0, 3))
stem("v4_k5_c8_516_units_on_512", V5, BF16, BF16, 129, 3, 5, 2, 32, 40, 8, units=516, grid=512, wrap=True)
stem("v4_k3_c4_260_units", V3, BF16, BF16, 65, 3, 3, 3, 32, 40, 4, lay=(4, 4), units=260, wrap=False)
# neighbours that must NOT be V4
stem("v4_not_w_in_12", SR("GENERIC", 1, 1, 1), BF16, BF16, 1, 3, 5, 2, 13, 12, 8)
stem("v4_not_cout_12", SR("GENERIC", 1, 1, 1), BF16, BF16, 1, 3, 5, 2, 13, 8, 12)
stem("v4_not_f32_source", SR("GENERIC", 1, 0, 1), BF16, F32, 1, 3, 5, 3, 13, 8, 8)

# ============================================================================= V2: whole tiles, reached at T == 1
# (an 18 x 22 output needs w_in 43 / 44, which the fast routes refuse (w_in % 8): 18 x 20 is the ragged frame here)
W5, W3 = SR("V2", 1, 1, 5), SR("V2", 1, 1, 3)
stem("v2_k5_c8_18x20", W5, BF16, BF16, 1, 3, 5, 1, 35, 40, 8, units=4, grid=4)
stem("v2_k3_c4_18x20_coff4", W3, BF16, BF16, 2, 3, 3, 1, 36, 40, 4, lay=(12, 4), units=8)
stem("v2_k3_c8_1x4", W3, BF16, BF16, 3, 3, 3, 1, 1, 8, 8, units=3)
stem("v2_k5_c8_260_units", W5, BF16, BF16, 65, 3, 5, 1, 35, 40, 8, units=260, grid=256, wrap=True)
stem("v2_k5_c4_tindex_one_frame", W5, BF16, BF16, 2, 3, 5, 4, 17, 24, 4, ti=(2,), lay=(4, 4), mem=("ntc", 8, 3))

# ============================================================================= S4: the slow stem (3 -> 64, kt 1)
# units as V4 with chunks of 2 pairs; ld and c_off multiples of 8
S4 = SR("S4", 1, 1, 1)
stem("s4_t2_7x4", S4, BF16, BF16, 1, 3, 1, 2, 13, 8, 64, units=1, grid=1)
stem("s4_t3_1x12", S4, BF16, BF16, 2, 3, 1, 3, 2, 24, 64, lay=(16, 8), units=2)
stem("s4_t5_9x20", S4, BF16, BF16, 1, 3, 1, 5, 17, 40, 64, units=4)                                       # nfull 2 and the half pair: one chunk
stem("s4_t7_17x12", S4, BF16, BF16, 1, 3, 1, 7, 33, 24, 64, units=6)                                       # two chunks
stem("s4_tindex_repeats_ntchw", S4, BF16, BF16, 2, 3, 1, 9, 17, 8, 64, ti=(8, 2, 2, 0, 5), mem=("ntc", 8, 2))
stem("s4_516_units_on_512", S4, BF16, BF16, 129, 3, 1, 2, 17, 40, 64, units=516, grid=512, wrap=True)
stem("s4_not_t1", SR("GENERIC", 1, 1, 4), BF16, BF16, 2, 3, 1, 1, 17, 24, 64)
stem("s4_not_ld_mod8_is_4", SR("GENERIC", 1, 1, 4), BF16, BF16, 1, 3, 1, 2, 13, 8, 64, lay=(12, 8))
stem("s4_not_cout32", SR("GENERIC", 1, 1, 2), BF16, BF16, 1, 3, 1, 3, 13, 24, 32)

# ============================================================================= GENERIC forward: 2 map x 2 source dtypes x FN 1 / 2 / 4
_GEO = {            # (cin, kt, mem)
    "c5k1": (5, 1, ("ntc", 21, 0)),       # the reference slow stem: a slice of 21-channel memory
    "c15k1": (15, 1, ("ntc", 21, 5)),     # the reference fast stem
    "c3k5": (3, 5, "nc"),
    "c2k3": (2, 3, "nc"),
    "c1k1": (1, 1, "nc"),
}
_GEN = [            # (geometry, map, source, cout, t, h_in, w_in)
    ("c5k1", BF16, BF16, 64, 2, 33, 13), ("c5k1", F32, F32, 20, 3, 13, 33), ("c5k1", BF16, F32, 4, 2, 17, 9),
    ("c15k1", BF16, BF16, 16, 2, 13, 35), ("c15k1", F32, BF16, 16, 1, 35, 13), ("c15k1", BF16, F32, 52, 2, 9, 9),
    ("c3k5", F32, F32, 16, 3, 13, 9), ("c3k5", BF16, F32, 32, 4, 9, 35), ("c3k5", F32, BF16, 4, 2, 35, 9),
    ("c2k3", BF16, BF16, 20, 3, 13, 13), ("c2k3", F32, F32, 16, 2, 9, 37), ("c2k3", F32, BF16, 52, 4, 13, 9),
    ("c1k1", F32, F32, 64, 2, 35, 37), ("c1k1", BF16, BF16, 32, 1, 13, 9), ("c1k1", F32, BF16, 32, 2, 9, 13),
    ("c1k1", BF16, F32, 20, 2, 9, 9), ("c2k3", BF16, F32, 64, 2, 9, 9), ("c5k1", BF16, F32, 16, 2, 9, 13),
]
for _g, _m, _s, _co, _t, _h, _w in _GEN:
    _cin, _kt, _mem = _GEO[_g]
    _fn = {1: 1, 2: 2, 3: 4, 4: 4}[(_co + 15) // 16]
    for _wg in (False, True):
        _bad = _wg and _m == BF16 and _co % 8                      # the filter gradient reads dy in 16-byte channel groups
        stem(f"{'wg' if _wg else 'gen'}_{_g}_{'bf16' if _m == BF16 else 'f32'}_from_{'bf16' if _s == BF16 else 'f32'}_co{_co}",
             SR("WG_GENERIC" if _wg else "GENERIC", int(_m == BF16), int(_s == BF16), _fn), _m, _s, 2, _cin, _kt, _t, _h, _w, _co,
             wg=_wg, mem=_mem, lay=(4, 4) if _m == F32 or _co % 8 else (8, 8), status=UNSUPPORTED if _bad else 0)
for _m in (BF16, F32):
    for _wg in (False, True):       # FN 3 has no instantiation: refused, nothing written
        stem(f"{'wg' if _wg else 'gen'}_cout36_{'bf16' if _m == BF16 else 'f32'}_refused", None, _m, _m, 1, 2, 3, 2, 9, 9, 36, wg=_wg,
             lay=(4, 4), status=UNSUPPORTED)
# LDS of the filter + patch: 15 planes with 16 channels in f32 need 144.6 KB (the opt-in above 64 KB), with 64 channels 312 KB
stem("gen_lds_145k_c15_f32_co16", SR("GENERIC", 0, 0, 1), F32, F32, 1, 15, 1, 2, 35, 13, 16, lay=(4, 4))
stem("gen_lds_158k_c15_bf16_co64", SR("GENERIC", 1, 1, 4), BF16, BF16, 1, 15, 1, 2, 13, 35, 64)
stem("gen_lds_312k_c15_f32_co64_refused", None, F32, F32, 1, 15, 1, 2, 13, 9, 64, lay=(4, 4), status=UNSUPPORTED)
stem("gen_4100_tiles_on_4096", SR("GENERIC", 1, 1, 1), BF16, BF16, 4100, 1, 1, 1, 1, 1, 8, units=4100, grid=4096, wrap=True)
stem("gen_1030_tiles_on_1024_lds_105k", SR("GENERIC", 0, 0, 4), F32, F32, 515, 5, 1, 2, 2, 1, 64, lay=(4, 4), units=1030, grid=1024,
     wrap=True)
stem("gen_1x1_output", SR("GENERIC", 0, 1, 2), F32, BF16, 1, 2, 3, 1, 1, 2, 24, lay=(4, 4), units=1, grid=1)
stem("gen_odd_w_in_sw2", SR("GENERIC", 1, 1, 1), BF16, BF16, 2, 3, 5, 3, 13, 23, 8, mem="w2")
stem("gen_tindex_backwards", SR("GENERIC", 0, 0, 1), F32, F32, 1, 5, 3, 6, 9, 13, 12, ti=(5, 5, 2, 0), mem=("ntc", 21, 3), lay=(4, 4))

# ============================================================================= WGV2: the fast stem's filter gradient
# items = clips x frames x 16 x 16 tiles, on at most 768 workgroups rounded up to a multiple of 8
WG = SR("WGV2", 1, 1, 0)
stem("wgv2_k1_t1_7x4", WG, BF16, BF16, 1, 3, 1, 1, 13, 8, 8, wg=True, units=1, grid=8)
stem("wgv2_k3_t1_17x20", WG, BF16, BF16, 1, 3, 3, 1, 33, 40, 8, wg=True, units=4, grid=8)                  # two of three temporal taps are padding
stem("wgv2_k5_t1_9x12_twice", WG, BF16, BF16, 3, 3, 5, 1, 17, 24, 8, wg=True, units=3, grid=8, twice=True)  # four of five are padding
stem("wgv2_k5_t2_18x20", WG, BF16, BF16, 2, 3, 5, 2, 35, 40, 8, wg=True, units=16, wrap=False)
stem("wgv2_k3_t6_17x12", WG, BF16, BF16, 1, 3, 3, 6, 33, 24, 8, wg=True, units=12, grid=16)                  # 4 surplus workgroups
stem("wgv2_k5_t6_tindex_repeat", WG, BF16, BF16, 2, 3, 5, 8, 13, 24, 8, wg=True, ti=(7, 2, 2, 0, 3, 3), mem=("ntc", 8, 2))
stem("wgv2_k1_t2_ntchw", WG, BF16, BF16, 2, 3, 1, 2, 17, 8, 8, wg=True, mem=("ntc", 5, 2), lay=(16, 8))
stem("wgv2_k5_792_items_on_768", WG, BF16, BF16, 33, 3, 5, 6, 33, 40, 8, wg=True, units=792, wrap=True)
stem("wgv2_k5_cout4_refused", None, BF16, BF16, 1, 3, 5, 2, 13, 8, 4, wg=True, lay=(12, 4), status=UNSUPPORTED)  # dy in 8-channel groups
stem("wgv2_not_coff4", None, BF16, BF16, 1, 3, 5, 2, 13, 8, 8, wg=True, lay=(12, 4), status=UNSUPPORTED)
stem("wgv2_not_kt7", SR("WG_GENERIC", 1, 1, 1), BF16, BF16, 1, 3, 7, 3, 13, 8, 8, wg=True)
stem("wgv2_f32_cout4", SR("WG_GENERIC", 0, 0, 1), F32, F32, 1, 3, 5, 2, 13, 8, 4, wg=True, lay=(4, 4))

# ============================================================================= WG_GENERIC: splits and pixel totals
# (blocks = pixel splits of a plane: min(ceil(2048 / planes), tiles), re-divided evenly)
stem("wg_one_pixel", SR("WG_GENERIC", 0, 0, 1), F32, F32, 1, 1, 1, 1, 1, 1, 4, wg=True, lay=(4, 4), units=1, grid=1)
stem("wg_255_pixels_two_tiles", SR("WG_GENERIC", 1, 1, 1), BF16, BF16, 1, 2, 3, 1, 29, 33, 8, wg=True, units=2, grid=2)
stem("wg_257_pixels", SR("WG_GENERIC", 0, 1, 2), F32, BF16, 1, 5, 1, 1, 1, 513, 24, wg=True, lay=(4, 4), units=17, grid=17)
stem("wg_many_tiles_per_split", SR("WG_GENERIC", 1, 0, 4), BF16, F32, 600, 15, 1, 1, 1, 1, 64, wg=True, units=600, grid=120, wrap=True)

# ============================================================================= sfk_stem2d_fwd / _wgrad
for _i, (_m, _s) in enumerate(((BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32))):
    for _j, ((_t, _c), (_h, _w)) in enumerate(zip(((1, 1), (10, 5), (3, 7)), ((1, 1), (33, 17), (39, 65)))):
        _co = (4, 36, 64)[(_i + _j) % 3]
        for _wg in (False, True):
            _bad = _m == BF16 and _co % 8                          # sfk_stem2d reads / writes its map in 16-byte channel groups
            stem2d(f"stem2d_{'wg' if _wg else 'fwd'}_{'bf16' if _m == BF16 else 'f32'}_from_{'bf16' if _s == BF16 else 'f32'}"
                   f"_t{_t}c{_c}_co{_co}", _m, _s, 2, _t, _c, _h, _w, _co, wg=_wg, lay=(4, 4) if _m == F32 else (8, 8),
                   status=UNSUPPORTED if _bad else 0)
stem2d("stem2d_fwd_bf16_co64_20x33", BF16, BF16, 1, 3, 7, 39, 65, 64)
stem2d("stem2d_wg_bf16_co8_1x1", BF16, F32, 3, 1, 1, 1, 1, 8, wg=True)
stem2d("stem2d_fwd_4097_planes_refused", F32, F32, 1, 4097, 1, 1, 1, 4, lay=(4, 4), status=UNSUPPORTED)
stem2d("stem2d_wg_4097_planes_refused", F32, F32, 1, 4097, 1, 1, 1, 4, wg=True, lay=(4, 4), status=UNSUPPORTED)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def bound(case: Case, be, dev="cpu"):
    """(StemSrc, map, signature) of the case bound on `be`"""
    rec = la.Recorder(be)
    p, m = case.bind(rec, dev)
    (sig,) = rec.calls
    return p, m, sig


def filled(sig, be, device, seed: int = 0):
    """the decoded arguments of a signature on launch_audit's seeded, guarded buffers, as replay() sets them up: (args, buffers)"""
    method, args, groups, _ = sig
    gen = torch.Generator(device=device).manual_seed(seed)
    bufs = la.Buffers(groups, device)
    la._fill(sig, bufs, gen)
    la._walk_ints(args, bufs)
    A = {k: la._decode(e, bufs) for k, e in args}
    la._prepare_inputs(method, A, gen, be)
    return A, bufs


def replay_refused(sig, be, device, seed: int = 0) -> Tuple[Optional[int], bool]:
    """run a call that must be refused on those buffers: (the sfk_status it raised or None, every byte of every buffer
    unchanged)"""
    A, bufs = filled(sig, be, device, seed)
    before = [v.clone() for v in bufs.views]
    status = None
    try:
        getattr(be, sig[0])(**A)(torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
    except SfkError as e:
        status = int(re.search(r"\((-?\d+)\)\s*$", str(e)).group(1))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return status, all(torch.equal(a, b) for a, b in zip(bufs.views, before))


# ============================================================================= the uint8 and pooled stems
@dataclasses.dataclass
class U8Case:
    name: str
    kind: str                        # "3d" | "2d"
    pool: bool
    wg: bool
    mdt: torch.dtype
    n: int
    t: int
    s: int                           # frames are s x s
    pitch: int
    c0: int
    c: int
    cout: int
    kt: int = 1
    crop: Optional[str] = None       # None | "zero" | "max" | "random"
    ti: Optional[Tuple[int, ...]] = None
    missing: Tuple[Tuple[int, int], ...] = ()     # pool: (clip, frame) entries of the index table that name no frame
    lay: Tuple[int, int] = (8, 8)
    seed: int = 0

    @property
    def method(self) -> str:
        return ("u8p" if self.pool else "u8") + ("stem2d_" if self.kind == "2d" else "stem_conv_") + ("wgrad" if self.wg else "fwd")

    @property
    def tag(self) -> str:
        """the source tag the entry point instantiates (csrc/stem_conv.hip, csrc/stem2d.hip): forward by x.c alone"""
        base = "PoolLut" if self.pool else "Lut"
        if self.wg or self.kind == "2d" or self.c not in (5, 15):
            return base
        return f"{'Pool' if self.pool else ''}Pix{self.c}"


U8: List[U8Case] = []
_CROPS = (None, "zero", "max", "random")
_i = 0
for _pool in (False, True):
    # forward: every source tag (x.c 5, 15, other) with 1, 2 and 4 channel fragments and both map dtypes; a pitch of 21 with a
    # channel offset and a pitch of exactly c.  (15 planes in f32 leave room for 16 channels in 160 KB of LDS.)
    for _c, _c0, _pitch, _m, _co, _kt in (
            (5, 0, 21, BF16, 8, 1), (5, 0, 5, F32, 32, 1), (5, 3, 21, BF16, 64, 3), (5, 0, 21, F32, 16, 3),
            (15, 5, 21, BF16, 32, 1), (15, 0, 15, F32, 16, 1), (15, 5, 21, BF16, 64, 1), (15, 0, 15, BF16, 8, 1),
            (3, 2, 5, BF16, 8, 3), (3, 0, 3, F32, 32, 1), (3, 2, 21, F32, 64, 1), (3, 2, 5, BF16, 64, 3)):
        _s = (18, 34, 70)[_i % 3]
        U8.append(U8Case(f"{'u8p' if _pool else 'u8'}_fwd_c{_c}_p{_pitch}_{'bf16' if _m == BF16 else 'f32'}_s{_s}_co{_co}_k{_kt}",
                         "3d", _pool, False, _m, 2, 4, _s, _pitch, _c0, _c, _co, _kt, _CROPS[_i % 4],
                         ti=(3, 0, 0) if _i % 5 == 1 else None, missing=((0, 0), (1, 3), (1, 2)) if _pool else (),
                         lay=(4, 4) if _m == F32 else (8, 8), seed=_i))
        _i += 1
    for _m, _c, _co, _kt, _s, _crop in ((BF16, 5, 64, 1, 18, "random"), (F32, 15, 20, 1, 34, "max"), (F32, 3, 4, 3, 18, None),
                                       (BF16, 3, 8, 3, 34, "zero")):
        U8.append(U8Case(f"{'u8p' if _pool else 'u8'}_wg_c{_c}_{'bf16' if _m == BF16 else 'f32'}_s{_s}_co{_co}_k{_kt}", "3d", _pool,
                         True, _m, 2, 3, _s, 21, 2, _c, _co, _kt, _crop, ti=(2, 0, 1, 1) if _kt == 3 else None,
                         missing=((1, 0),) if _pool else (), lay=(4, 4) if _m == F32 else (8, 8), seed=40 + _i))
        _i += 1
    for _m, _wg, _t, _c, _co, _s, _pitch, _crop in ((BF16, False, 10, 5, 64, 34, 21, "random"), (F32, False, 3, 7, 36, 18, 7, "max"),
                                                  (BF16, True, 3, 7, 8, 18, 21, None), (F32, True, 10, 5, 4, 70, 5, "zero")):
        U8.append(U8Case(f"{'u8p' if _pool else 'u8'}_2d_{'wg' if _wg else 'fwd'}_t{_t}c{_c}_{'bf16' if _m == BF16 else 'f32'}_s{_s}_co{_co}",
                         "2d", _pool, _wg, _m, 2, _t, _s, _pitch, 0, _c, _co, _t, _crop, missing=((0, 1),) if _pool else (),
                         lay=(4, 4) if _m == F32 else (8, 8), seed=80 + _i))
        _i += 1
U8_BY_NAME = {c.name: c for c in U8}
assert len(U8_BY_NAME) == len(U8)


def u8_source(c: U8Case, dev, crop_delta: int = 0):
    """the U8Clip / PoolClip of the case on `dev` (seeded on the CPU) and the float clip it stands for, (N, c, T, H, W) f32 on
    `dev`, materialised on the CPU by the emulations' statement of the headers' formula.  crop_delta shifts the crop the
    KERNEL side sees (a mutation)"""
    import emu_u8stem
    import emu_u8stem_pool
    g = torch.Generator().manual_seed(1000 + c.seed)
    pad = c.s // 10
    lut = normalize_lut()
    crop = None
    if c.crop == "zero":
        crop = torch.zeros(c.n, 2, dtype=torch.int32)
    elif c.crop == "max":
        crop = torch.full((c.n, 2), 2 * pad, dtype=torch.int32)
    elif c.crop == "random":
        crop = torch.randint(0, 2 * pad + 1, (c.n, 2), generator=g, dtype=torch.int32)
    if c.pool:
        nf = c.n * c.t + 3
        arena = torch.randint(0, 256, (nf, c.s, c.s, c.pitch), generator=g, dtype=torch.uint8)
        index = torch.randperm(nf, generator=g)[: c.n * c.t].to(torch.int32).view(c.n, c.t).contiguous()
        for i, (a, b) in enumerate(c.missing):
            index[a, b] = (-1, nf, -7)[i % 3]
        make = lambda a, i, cr, l: PoolClip(a, i, c.c0, c.c, cr, pad, l, 37)                      # noqa: E731
        x_cpu = make(arena, index, crop, lut)
        x = emu_u8stem_pool.materialize(x_cpu)
        shifted = None if crop is None else (crop + crop_delta).to(dev)
        clip = make(arena.to(dev), index.to(dev), shifted, lut.to(dev))
    else:
        frames = torch.randint(0, 256, (c.n, c.t, c.s, c.s, c.pitch), generator=g, dtype=torch.uint8)
        x = emu_u8stem.materialize(U8Clip(frames, c.c0, c.c, crop, pad, lut))
        shifted = None if crop is None else (crop + crop_delta).to(dev)
        clip = U8Clip(frames.to(dev), c.c0, c.c, shifted, pad, lut.to(dev))
    return clip, x.contiguous().to(dev)


def u8_run(c: U8Case, be, dev, crop_delta: int = 0, float_be=None) -> Tuple[la.Replay, Optional[bool]]:
    """one uint8 / pooled stem call on guarded, seeded buffers, held to launch_audit's float64 restatement of the float stem
    over the materialised clip: the Replay, and -- with float_be -- whether the float entry point on that clip gives the
    same bits (forward map and statistics; the filter gradients add with atomics and are both held to float64 instead)"""
    two_d = c.kind == "2d"
    clip, x = u8_source(c, dev, crop_delta)
    ti = None if c.ti is None or two_d else torch.tensor(c.ti, dtype=torch.int32, device=dev)
    kt = c.t if two_d else c.kt
    pu, pf = StemSrc(clip, ti, kt), StemSrc(x, ti, kt)
    t_out = 1 if two_d else pu.t_len
    ho = _out(c.s)
    kp = stem_kp(c.c, kt)
    ld = c.cout + c.lay[0]
    es = 2 if c.mdt == BF16 else 4
    rows = c.n * t_out * ((ho + 15) // 16) ** 2
    # groups: 0 the map, 1 the filter / dw, 2 stats -- each at 16 modulo 256 with launch_audit's guard behind it
    groups = ((16, c.n * t_out * ho * ho * ld * es), (16, c.cout * kp * (4 if c.wg else es)), (16, (rows + 2) * c.cout * 2 * 4))
    gen = torch.Generator(device=dev).manual_seed(c.seed)

    def decode(b):
        m = FMap(b.typed(0, 0, c.mdt, c.n * t_out * ho * ho * ld), c.n, t_out, ho, ho, c.cout, ld, c.lay[1])
        if c.wg:
            return {"dy": m, "dw": b.typed(1, 0, F32, c.cout * kp)}
        return {"w": b.typed(1, 0, c.mdt, c.cout * kp), "y": m, "stats": b.typed(2, 0, F32, (rows + 2) * c.cout * 2)}
    bufs = la.Buffers(groups, dev)
    for v, dt in zip(bufs.views, (c.mdt, F32 if c.wg else c.mdt, F32)):
        k = v.numel() // (2 if dt == BF16 else 4)
        v[: k * (2 if dt == BF16 else 4)].view(dt).copy_(torch.randn(k, generator=gen, device=dev).to(dt))
    A = decode(bufs)
    if not c.wg:
        la._prepare_inputs("stem2d_fwd" if two_d else "stem_conv_fwd", {"p": pf, **A}, gen, be)
    before = la.Buffers(groups, dev)
    for b, a in zip(before.views, bufs.views):
        b.copy_(a)
    B = {"p": pf, **decode(before)}
    stream = torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else 0
    getattr(be, c.method)(pu, **A)(stream)
    same = None
    if float_be is not None and not c.wg:
        twin = la.Buffers(groups, dev)
        for b, a in zip(twin.views, before.views):
            b.copy_(a)
        getattr(float_be, "stem2d_fwd" if two_d else "stem_conv_fwd")(pf, **decode(twin))(stream)
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)
    if float_be is not None and not c.wg:
        same = all(torch.equal(a, b) for a, b in zip(twin.views, bufs.views))
    ref = la._ref_stem_wgrad if c.wg else la._ref_stem_fwd
    outs = ref(be, B, two_d=two_d)
    verdicts = []
    for o in outs:
        if o.ref is None:
            continue
        got = o.view(A)
        if o.exact:
            gd = got.to(ref64.F64)
            ok = (gd == o.ref) | (o.alt_mask & (gd == o.alt))
            bad = int((~ok).sum())
            verdicts.append(ref64.Verdict(o.name, o.kind, 0.0 if bad == 0 else float("inf"), 0.0, 1.0, gd.numel()))
        else:
            verdicts.append(ref64.judge(o.name, got, o.ref, o.a, o.k, o.dtype, o.kind))
    after = la.Buffers(groups, dev)
    for b, a in zip(after.views, bufs.views):
        b.copy_(a)
    Aft = decode(after)
    for o in outs:
        o.view(Aft).copy_(o.view(B))
    bad = [i for i, (p, q) in enumerate(zip(after.views, before.views)) if not torch.equal(p, q)]
    return la.Replay(None, None, verdicts, not bad, bad, None, 0.0, A), same
