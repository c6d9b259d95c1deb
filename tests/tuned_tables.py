"""TEST INFRASTRUCTURE: three non-default sfk_tuning tables and what every edge case must report under each of them
(tests/tuned_worker.py runs one table per child process; tests/test_tuned_routes_cpu.py and tests/test_gpu_tuned_routes.py
read what it writes).  No GPU import.

The tuning table is write-once per process, so the suite's own process only ever launches what the DEFAULT table reaches.
A table here is a dict of the environment names of _lib.TUNING_ENV; the worker is started with exactly these set:
  narrow  16-byte epilogue stores off: the 4-channel store path of every fused epilogue.
  alt     the instantiations only a knob reaches: the 224-row P8 tile, the four-co-group pointwise kernel, the 5-slot ring of
          the LDS-DMA filter gradient, the whole-tile stem forward at T > 1, the cached bn_apply and the streaming reduce /
          bwd_apply at small maps, a second trip of the pooling grids, a partial-row cap that does not divide by two chunks.
  off     every specialised kernel switched off: listed routes at shapes they have never been held at.
For each table this module names, by case name, every case of conv_edges.CASES / stem_edges.CASES whose report (route,
workspace flag, splits, units, grid) differs from its default declaration, with the values it must report there -- taken
ONCE from the CPU route queries (`python tests/tuned_worker.py TABLE routes OUT`), then pinned: nothing is computed at test
time.  A case that is not named must report its default declaration unchanged.  The case objects are conv_edges' and
stem_edges' own; the new cases are made by the same constructors."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional

import torch

import bn_ref64 as B
import conv_edges as E
import head_ref64 as H
import stem_edges as S
from conv_edges import BF16, F32, IR, PW, WR

COGROUPS4 = 1 << 29        # SFK_IGEMM_ROUTE_COGROUPS4 of include/sfk.h
RING5 = 1 << 30            # SFK_WGRAD_ROUTE_RING5

BN_PARTS = 37              # below 1024; 37 // 2 = 18 rows for two channel chunks, with a remainder
POOL_BLOCKS = 2            # 512 threads per trip of the pooling grids
SMALL_K = 4096             # above every case's K = taps x cin (the largest: 27 x 40 = 1080)

TABLES: Dict[str, Dict[str, int]] = {
    "narrow": {"SFK_WIDE": 0},
    "alt": {"SFK_P8": 3, "SFK_PW_STREAM": 2, "SFK_WG_WIDECO": 15, "SFK_STEM3": 0, "SFK_NT_APPLY_MB": -1, "SFK_NT_RED_MB": 0,
            "SFK_NT_BAPP_MB": 0, "SFK_POOL_BLOCKS": POOL_BLOCKS, "SFK_BN_PARTS": BN_PARTS},
    "off": {"SFK_P8": 0, "SFK_TILE256": 1, "SFK_HALO": 0, "SFK_WGBAND": 0, "SFK_WGP8": 0, "SFK_WGWS_LIB": 0, "SFK_WG_WIDECO": 0,
            "SFK_PW_STREAM": 0, "SFK_SMALLK": SMALL_K, "SFK_KSHORT": 0, "SFK_NT_RED_MB": -1, "SFK_NT_BAPP_MB": -1},
}
DEFAULT = "default"        # no knob: the worker accepts it as the baseline when the pins below are regenerated


def env_of(table: str) -> Dict[str, str]:
    return {} if table == DEFAULT else {k: str(v) for k, v in TABLES[table].items()}


# ============================================================================= new cases
def _new(make, *a, slow=False, **kw):
    """a case made by one of conv_edges' constructors, taken back out of ITS table (conv_edges.CASES stays the default's)"""
    n = len(E.CASES)
    make(*a, **kw)
    (case,) = E.CASES[n:]
    del E.CASES[n:]
    case.slow = slow
    return case


_EP256 = ("scale", "shift", "res", "res_scale", "res_shift", "relu", "relu_bits")
P8_224, P8_256 = IR("P8", 1, 224, 256, 0, 0, 1), IR("P8", 1, 256, 256, 0, 0, 1)
R5_128, R5_256 = WR("DMA", 1, 128, 128, 4) | RING5, WR("DMA", 1, 256, 128, 8) | RING5
# the 8-wave ring needs cout >= 256 and M x cols >= 2^24: with cols = 128 and ONE dW tile the 192 pixel splits take
# ceil(chunks / 192) chunks of 32 pixels each and the last split the remainder (the arithmetic of launch_dma, restated in
# ring_runs below): M = 131,072 + 32 r' gives the last split a run of 1 .. 4 chunks, shorter than the 5 slots
NEW: Dict[str, List[E.Case]] = {
    "narrow": [],
    "alt": [
        # ---- the 224-row P8 tile: float64 on the CPU takes minutes at K = 1024 (route and geometry only there, as SLOW_ON_CPU)
        _new(E.conv, "p8_224_cout512_two_column_tiles", P8_224, BF16, 1, PW(16385), 1024, 512, yl=(8, 8), slow=True),
        _new(E.conv, "p8_224_exactly_256_tiles_bits_acc", IR("P8", 1, 224, 256, 2, 0, 1), BF16, 1, PW(57344), 1024, 256, obits=True,
             acc=True, slow=True),
        _new(E.conv, "p8_257_tiles_of_224_stay_on_256_rows", P8_256, BF16, 1, PW(57345), 1024, 256, slow=True),
        # ---- the four-co-group pointwise kernel (1 and 777 pixels and a sliced y: the existing cases, which move to it)
        _new(E.conv, "bf16_pw_cg4_4097_px", IR("PWF", 1, 64, 256, 0, 0, 1) | COGROUPS4, BF16, 1, PW(4097), 64, 256, ep=_EP256,
             xl=(8, 0), yl=(24, 16), rl=(8, 8)),
        # ---- the 5-slot ring, 4-wave tile: runs of 1 .. 6 chunks in ONE split; workspace and atomics alternate
        *[_new(E.wgrad, f"wg_ring5_128_run{j + 1}", R5_128, BF16, 1, PW(32 * j + 1), 136, 136, ws="full" if j % 2 else None,
               many=False, xl=(8, 8) if j % 3 == 0 else (0, 0), dl=(8, 0) if j % 3 == 1 else (0, 0)) for j in range(6)],
        # ---- 8-wave tile, 192 splits: the last split's run is 1 / 2 / 4 chunks (the others 22)
        _new(E.wgrad, "wg_ring5_256_last_run1", R5_256, BF16, 1, PW(22 * 191 * 32 + 1), 128, 256, many=True),
        _new(E.wgrad, "wg_ring5_256_last_run2_atomics", R5_256, BF16, 1, PW(22 * 191 * 32 + 33), 128, 256, ws=None, many=True),
        _new(E.wgrad, "wg_ring5_256_last_run4", R5_256, BF16, 1, PW(22 * 191 * 32 + 97), 128, 256, many=True, xl=(8, 8)),
        # ---- the partial-row cap of the BatchNorm reductions binds (37 rows; 18 with two channel chunks)
        *[_new(E.bn, f"bn_{m}_{t}_g{g}_px{px}_capped", f"bn_{m}", dt, g * v, 1, (1, 1, px), 1024, flavour=fl, lay=(v, v))
          for m, fl in (("stats", 0), ("bwd_reduce", 1))
          for dt, t, v in ((BF16, "bf16", 8), (F32, "f32", 4))
          for g, px in ((10, 25 * 16 * 37 + 1), (256, 16 * 37 + 1), (288, 16 * 18 + 1))],
    ],
    "off": [],
}
NEW_BY_NAME = {t: {c.name: c for c in cs} for t, cs in NEW.items()}


def ring_runs(m: int, tiles: int, target: int) -> List[int]:
    """chunks per pixel split of the LDS-DMA filter gradient (csrc/conv_wgrad.hip launch_dma, restated): `tiles` dW tiles,
    workgroup target `target` (192 for the 8-wave tile, 256 for the 4-wave one)"""
    chunks = -(-m // 32)
    splits = max(1, min(-(-target // tiles), (chunks + 7) // 8, 65535))
    per = -(-chunks // splits)
    splits = -(-chunks // per)
    return [per] * (splits - 1) + [chunks - per * (splits - 1)]


# what the new ring cases are about, stated from their shapes: (case, dW tiles, target) -> the runs
RING_RUNS = {f"wg_ring5_128_run{j + 1}": (4, 256, [j + 1]) for j in range(6)}
RING_RUNS.update({"wg_ring5_256_last_run1": (1, 192, [22] * 191 + [1]), "wg_ring5_256_last_run2_atomics": (1, 192, [22] * 191 + [2]),
                  "wg_ring5_256_last_run4": (1, 192, [22] * 191 + [4])})


# ============================================================================= BatchNorm partial rows and cache hints
def nparts_rule(cgs: int, pixels: int, max_parts: int, bn_parts: int) -> int:
    """include/sfk.h / csrc/bn.hip chan_grid restated: >= 16 pixels per thread, at most bn_parts divided by the channel
    chunks of 256 groups (at least 1), at most max_parts"""
    rows_b = 256 // min(cgs, 256)
    parts = -(-pixels // (rows_b * 16))
    parts = min(parts, max(1, bn_parts // (-(-cgs // 256))))
    if max_parts > 0:
        parts = min(parts, max_parts)
    return max(1, parts)


def nt_rule(map_bytes: int, mb: int) -> bool:
    """the streaming (non-temporal) instantiation runs for maps of >= mb MB; -1: never"""
    return mb >= 0 and map_bytes >= (mb << 20)


# the instantiation every case of the BatchNorm tables takes under the table (the maps here are far below 1 MB, so a
# threshold of 0 streams every one of them and the default 48 / 150 MB none)
NT = {"alt": {"bn_apply": False, "bn_bwd_reduce": True, "bn_bwd_apply": True}}
NT_FIELD = {"bn_apply": "nt_apply_mb", "bn_bwd_reduce": "nt_reduce_mb", "bn_bwd_apply": "nt_bwd_apply_mb"}
BN_METHODS = ("bn_stats", "bn_bwd_reduce", "bn_maxpool_fwd", "bn_maxpool_bwd_reduce", "bn_maxpool_bwd_apply")


# ============================================================================= pooling grids at pool_blocks = 2
def _pool(dtype, k, s, p, h, w, n=1, t=1, cg=1):
    return dict(dtype=dtype, k=k, s=s, p=p, h=h, w=w, fill="mixed", n=n, t=t, cg=cg)


def pool_items(case) -> Dict[str, int]:
    """items (threads needed) of the forward (output elements / vector) and the backward (input elements / vector) launch"""
    k, s, p, h, w = case["k"], case["s"], case["p"], case["h"], case["w"]
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    m = case["n"] * case["t"] * case["cg"]
    return {"fwd": m * ho * wo, "bwd": m * h * w}


# (case, trips of the forward grid, trips of the backward grid) with 2 x 256 threads per trip: the count is ceil(items / 512)
POOL_CASES = [
    (_pool(BF16, 3, 2, 1, 31, 63), 1, 4),            # fwd 16 x 32 = exactly 512 items; bwd 1953 = three trips + 417
    (_pool(F32, 3, 2, 1, 37, 53), 2, 4),             # fwd 19 x 27 = 513: one thread of a second trip
    (_pool(BF16, 3, 2, 1, 16, 32), 1, 1),            # bwd exactly 512
    (_pool(F32, 3, 2, 1, 19, 27), 1, 2),             # bwd 513
    (_pool(BF16, 3, 2, 1, 69, 87), 4, 12),           # fwd 35 x 44 = 1540 = three trips + 4
    (_pool(F32, 3, 1, 1, 16, 32), 1, 1),             # the general window keeps the frame: fwd = bwd = 512
    (_pool(BF16, 3, 1, 1, 9, 19, cg=3), 2, 2),       # 513 = 171 pixels x 3 groups: the trip boundary inside a pixel
    (_pool(F32, 5, 3, 2, 103, 43, n=2), 3, 18),      # fwd 2 x 35 x 15 = 1050 = two trips + 26; bwd 8858
    (_pool(BF16, 2, 2, 0, 70, 88), 4, 13),      # fwd 1540
]


def pool_name(case) -> str:
    return B.pool_name(case) + f"-n{case['n']}t{case['t']}g{case['cg']}"


# the head's general-window backward (items = elements of dx) and its dropout mask (items = n x c x window positions) take
# their grids from the same cap: (case of head_ref64.check_pool, trips of the backward, trips of the mask launch)
def _head(name, dtype, n, c, dims, k):
    return H._pool(f"{name}-n{n}c{c}-{'x'.join(map(str, dims))}-k{'x'.join(map(str, k))}", dtype, n, 0.5, [H._part(c, dims, k=k, f_off=4)])


def head_items(case) -> Dict[str, int]:
    (p,) = case["parts"]
    pos = math.prod(H.positions(p["dims"], p["k"]))
    return {"bwd": case["n"] * math.prod(p["dims"]) * p["c"], "mask": case["n"] * p["c"] * pos}


HEAD_POOL_CASES = [            # (bf16 only from 2048 elements on: below that a bf16 map's aggregate ratio says nothing, ref64.SMALL_MAP)
    (_head("f32", F32, 1, 8, (4, 4, 4), (2, 2, 2)), 1, 1),            # bwd 64 pixels x 8 = exactly 512; mask 8 x 27
    (_head("f32", F32, 1, 9, (3, 19, 1), (1, 1, 1)), 2, 2),           # bwd 57 x 9 = 513 and mask 9 x 57 = 513
    (_head("f32", F32, 1, 8, (5, 5, 5), (2, 2, 2)), 2, 1),            # mask 8 x 64 = exactly 512; bwd 1000
    (_head("bf16", BF16, 1, 12, (3, 3, 19), (2, 2, 2)), 5, 2),        # bwd 171 x 12 = 2052 = four trips + 4; mask 12 x 72 = 864
    (_head("bf16", BF16, 2, 24, (6, 4, 4), (4, 2, 2)), 9, 3),         # bwd 4608 = nine whole trips; mask 2 x 24 x 27 = 1296
]


# ============================================================================= the pins
# name -> route                                   (sfk_conv_igemm)
# name -> (route, workspace path, pixel splits)   (sfk_conv_wgrad)
# name -> (route, units, grid)                    (the stems)
MOVED_CONV: Dict[str, Dict[str, int]] = {"narrow": {}, "alt": {}, "off": {}}
MOVED_WGRAD: Dict[str, Dict[str, tuple]] = {"narrow": {}, "alt": {}, "off": {}}
MOVED_STEM: Dict[str, Dict[str, tuple]] = {"narrow": {}, "alt": {}, "off": {}}
_SR = S.SR
MOVED_CONV["narrow"]["bf16_reg64_wide_stride2"] = IR("REG", 1, 256, 64, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_reg64_more_tiles_than_resident"] = IR("REG", 1, 256, 64, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_reg32_long_wide"] = IR("REG", 1, 256, 32, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_reg32_short_wide"] = IR("REG", 1, 256, 32, 0, 1, 0)
MOVED_CONV["narrow"]["bf16_dma128_wide_last_row"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma128_one_pixel"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma128_dgrad_s2_pass0"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma128_dgrad_s2_pass3"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma256x128_wide"] = IR("DMA", 1, 256, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma_t256_224_wide"] = IR("DMA", 1, 224, 256, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_dma_t256_256_wide"] = IR("DMA", 1, 256, 256, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_p8_256"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_halo_one_band"] = IR("REG", 1, 256, 64, 0, 0, 0)
MOVED_CONV["narrow"]["bf16_halo_258_bands_perm"] = IR("REG", 1, 256, 64, 0, 0, 0)
MOVED_CONV["alt"]["bf16_p8_256"] = IR("P8", 1, 224, 256, 0, 0, 1)
MOVED_CONV["alt"]["bf16_p8_256_bits_acc"] = IR("P8", 1, 224, 256, 2, 0, 1)
MOVED_CONV["alt"]["bf16_pw_fused_40_256"] = IR("PWF", 1, 64, 256, 0, 0, 1) | COGROUPS4
MOVED_CONV["alt"]["bf16_pw_fused_one_pixel"] = IR("PWF", 1, 64, 256, 0, 0, 1) | COGROUPS4
MOVED_WGRAD["alt"]["wg_bf16_dma128_ws"] = (WR("DMA", 1, 128, 128, 4, 0, 0) | RING5, True, 1)
MOVED_WGRAD["alt"]["wg_bf16_dma128_small_ws"] = (WR("DMA", 1, 128, 128, 4, 0, 0) | RING5, False, 9)
MOVED_WGRAD["alt"]["wg_bf16_dma128_atomics_taps"] = (WR("DMA", 1, 128, 128, 4, 0, 0) | RING5, False, 1)
MOVED_WGRAD["alt"]["wg_bf16_dma128_one_pixel"] = (WR("DMA", 1, 128, 128, 4, 0, 0) | RING5, True, 1)
MOVED_WGRAD["alt"]["wg_bf16_dma256_big"] = (WR("DMA", 1, 256, 128, 8, 0, 0) | RING5, True, 48)
MOVED_STEM["alt"]["v4_k5_c8_t2_7x4"] = (_SR("V2", 1, 1, 5), 1, 1)
MOVED_STEM["alt"]["v4_k5_c4_t3_1x12_coff4"] = (_SR("V2", 1, 1, 5), 2, 2)
MOVED_STEM["alt"]["v4_k3_c8_t17_9x20"] = (_SR("V2", 1, 1, 3), 4, 4)
MOVED_STEM["alt"]["v4_k3_c4_t19_17x12"] = (_SR("V2", 1, 1, 3), 4, 4)
MOVED_STEM["alt"]["v4_k5_c8_t35_7x4"] = (_SR("V2", 1, 1, 5), 3, 3)
MOVED_STEM["alt"]["v4_k5_c8_t19_9x4"] = (_SR("V2", 1, 1, 5), 2, 2)
MOVED_STEM["alt"]["v4_k3_c8_t2_17x20"] = (_SR("V2", 1, 1, 3), 12, 12)
MOVED_STEM["alt"]["v4_k5_c8_tindex_repeats"] = (_SR("V2", 1, 1, 5), 2, 2)
MOVED_STEM["alt"]["v4_k3_c4_tindex_long_clip"] = (_SR("V2", 1, 1, 3), 1, 1)
MOVED_STEM["alt"]["v4_k5_c8_ntchw_slice"] = (_SR("V2", 1, 1, 5), 2, 2)
MOVED_STEM["alt"]["v4_k3_c8_ntchw_slice_tindex"] = (_SR("V2", 1, 1, 3), 2, 2)
MOVED_STEM["alt"]["v4_k5_c8_516_units_on_512"] = (_SR("V2", 1, 1, 5), 258, 256)
MOVED_STEM["alt"]["v4_k3_c4_260_units"] = (_SR("V2", 1, 1, 3), 130, 130)
MOVED_STEM["alt"]["s4_t2_7x4"] = (_SR("GENERIC", 1, 1, 4), 2, 2)
MOVED_STEM["alt"]["s4_t3_1x12"] = (_SR("GENERIC", 1, 1, 4), 6, 6)
MOVED_STEM["alt"]["s4_t5_9x20"] = (_SR("GENERIC", 1, 1, 4), 10, 10)
MOVED_STEM["alt"]["s4_t7_17x12"] = (_SR("GENERIC", 1, 1, 4), 14, 14)
MOVED_STEM["alt"]["s4_tindex_repeats_ntchw"] = (_SR("GENERIC", 1, 1, 4), 10, 10)
MOVED_STEM["alt"]["s4_516_units_on_512"] = (_SR("GENERIC", 1, 1, 4), 516, 516)
MOVED_CONV["off"]["f32_reg32_short_k5"] = IR("REG", 0, 256, 32, 0, 0, 0)
MOVED_CONV["off"]["f32_reg16_short_one_pixel"] = IR("REG", 0, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["f32_reg16_short_4ch"] = IR("REG", 0, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["f32_reg16_lateral_7"] = IR("REG", 0, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["bf16_reg32_short_wide"] = IR("REG", 1, 256, 32, 0, 0, 1)
MOVED_CONV["off"]["bf16_reg32_short_narrow_k5"] = IR("REG", 1, 256, 32, 0, 0, 0)
MOVED_CONV["off"]["bf16_reg16_short_one_pixel"] = IR("REG", 1, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["bf16_reg16_short_12ch_acc"] = IR("REG", 1, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["bf16_reg16_lateral_4"] = IR("REG", 1, 256, 16, 0, 0, 0)
MOVED_CONV["off"]["bf16_dma256x128_wide"] = IR("DMA", 1, 128, 128, 0, 0, 1)
MOVED_CONV["off"]["bf16_dma256x128_narrow"] = IR("DMA", 1, 128, 128, 0, 0, 0)
MOVED_CONV["off"]["bf16_dma_t256_224_wide"] = IR("DMA", 1, 256, 256, 0, 0, 1)
MOVED_CONV["off"]["bf16_dma_t256_224_narrow"] = IR("DMA", 1, 256, 256, 0, 0, 0)
MOVED_CONV["off"]["bf16_dma256x128_bits"] = IR("DMA", 1, 128, 128, 2, 0, 1)
MOVED_CONV["off"]["bf16_dma256x128_ep_relu"] = IR("DMA", 1, 128, 128, 3, 0, 1)
MOVED_CONV["off"]["bf16_p8_256"] = IR("DMA", 1, 128, 128, 0, 0, 1)
MOVED_CONV["off"]["bf16_p8_256_bits_acc"] = IR("DMA", 1, 128, 128, 2, 0, 1)
MOVED_CONV["off"]["bf16_halo_one_band"] = IR("REG", 1, 256, 64, 0, 0, 1)
MOVED_CONV["off"]["bf16_halo_258_bands_perm"] = IR("REG", 1, 256, 64, 0, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_8_32"] = IR("REG", 1, 256, 32, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_24_64"] = IR("REG", 1, 256, 64, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_40_64"] = IR("REG", 1, 256, 64, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_32_128"] = IR("DMA", 1, 128, 128, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_104_128"] = IR("DMA", 1, 128, 128, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_40_256"] = IR("DMA", 1, 128, 128, 4, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_104_320"] = IR("DMA", 1, 128, 128, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_128_512"] = IR("DMA", 1, 128, 128, 4, 0, 1)
MOVED_CONV["off"]["bf16_pw_fused_one_pixel"] = IR("DMA", 1, 128, 128, 4, 0, 1)
MOVED_CONV["off"]["bf16_pw_plain_64_acc"] = IR("REG", 1, 256, 64, 0, 0, 1)
MOVED_CONV["off"]["bf16_pw_plain_128_bias_acc"] = IR("DMA", 1, 128, 128, 3, 0, 1)
MOVED_CONV["off"]["bf16_pw_plain_320"] = IR("DMA", 1, 128, 128, 0, 0, 1)
MOVED_CONV["off"]["bf16_pw_dgrad_64_256"] = IR("DMA", 1, 128, 128, 5, 0, 1)
MOVED_CONV["off"]["bf16_pw_dgrad_128_512"] = IR("DMA", 1, 128, 128, 5, 0, 1)
MOVED_WGRAD["off"]["wg_f32_32x32_one_pixel"] = (WR("CFG", 0, 32, 32, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_f32_128x32_many"] = (WR("CFG", 0, 128, 32, 2, 0, 0), False, 17)
MOVED_WGRAD["off"]["wg_f32_64x128_9taps"] = (WR("CFG", 0, 64, 128, 2, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_f32_128x128_m65"] = (WR("CFG", 0, 128, 128, 1, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_f32_gram32"] = (WR("CFG", 0, 32, 32, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_f32_gram64"] = (WR("CFG", 0, 64, 128, 2, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_f32_gram128"] = (WR("CFG", 0, 128, 128, 1, 0, 0), False, 33)
MOVED_WGRAD["off"]["wg_bf16_32x32_one_pixel"] = (WR("CFG", 1, 32, 32, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_128x32_many"] = (WR("CFG", 1, 128, 32, 2, 0, 0), False, 17)
MOVED_WGRAD["off"]["wg_bf16_64x128_9taps"] = (WR("CFG", 1, 64, 128, 2, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_128x128_m65"] = (WR("CFG", 1, 128, 128, 1, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_gram32"] = (WR("CFG", 1, 32, 32, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_gram64"] = (WR("CFG", 1, 64, 128, 2, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_gram128"] = (WR("CFG", 1, 128, 128, 1, 0, 0), False, 33)
MOVED_WGRAD["off"]["wg_bf16_256x64_ragged"] = (WR("CFG", 1, 128, 128, 1, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_dma128_ws"] = (WR("DMA", 1, 128, 128, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_dma128_one_pixel"] = (WR("DMA", 1, 128, 128, 4, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_dma256_cols64"] = (WR("CFG", 1, 128, 128, 1, 0, 0), False, 17)
MOVED_WGRAD["off"]["wg_bf16_dma256_cols64_atomics"] = (WR("CFG", 1, 128, 128, 1, 0, 0), False, 1)
MOVED_WGRAD["off"]["wg_bf16_dma256_big"] = (WR("DMA", 1, 256, 128, 8, 0, 0), False, 48)
MOVED_WGRAD["off"]["wg_bf16_dma256_dg_slice"] = (WR("DMA", 1, 256, 128, 8, 0, 1), False, 1)
MOVED_WGRAD["off"]["wg_bf16_p8_ragged"] = (WR("DMA", 1, 256, 128, 8, 0, 0), False, 24)
MOVED_WGRAD["off"]["wg_bf16_band56_65_bands"] = (WR("CFG", 1, 64, 128, 2, 0, 0), False, 57)
MOVED_WGRAD["off"]["wg_bf16_band28_65_bands"] = (WR("DMA", 1, 128, 128, 4, 0, 0), False, 29)
MOVED_WGRAD["off"]["wg_bf16_band56_small_ws_falls_back"] = (WR("CFG", 1, 64, 128, 2, 0, 0), False, 57)


def conv_cases(table: str) -> List[E.Case]:
    """every conv / filter-gradient / BatchNorm-reduction case the table binds: conv_edges' own, then the new ones"""
    return list(E.CASES) + NEW.get(table, [])


def expected(table: str, case) -> dict:
    """what the case must report under the table"""
    if isinstance(case, S.Case):
        if case.status < 0 or case.route is None:
            return {"status": case.status}
        if case.name in MOVED_STEM.get(table, {}):
            r, u, g = MOVED_STEM[table][case.name]
            return {"status": 0, "route": r, "units": u, "grid": g}
        return {"status": 0, "route": case.route, "units": case.units, "grid": case.grid, "wrap": case.wrap}
    if case.method == "conv_igemm":
        return {"route": MOVED_CONV.get(table, {}).get(case.name, case.route)}
    if case.method == "conv_wgrad":
        if case.name in MOVED_WGRAD.get(table, {}):
            r, ws, sp = MOVED_WGRAD[table][case.name]
            return {"route": r, "ws": ws, "splits": sp}
        return {"route": case.route, "ws": case.ws, "many": case.many_splits}
    return {}


def check_line(table: str, case, ln: dict) -> list:
    """every way the worker's line for `case` differs from tuned_tables' declaration"""
    want, bad = expected(table, case), []
    if isinstance(case, S.Case):
        if case.method.startswith("stem2d"):
            return []
        if ln["status"] != want["status"]:
            return [("status", ln["status"], want["status"])]
        if "route" not in want:
            return []
        if ln["route"] != want["route"]:
            bad.append(("route", S.route_name(ln["route"]), S.route_name(want["route"])))
        for f in ("units", "grid"):
            if want.get(f) is not None and ln[f] != want[f]:
                bad.append((f, ln[f], want[f]))
        if want.get("wrap") is not None and (ln["units"] > ln["grid"]) != want["wrap"]:
            bad.append(("wrap", ln["units"], ln["grid"]))
        return bad
    if case.method == "conv_igemm":
        r = ln["route"]
        if r != want["route"]:
            bad.append(("route", E.route_name(r), E.route_name(want["route"])))
        kern, bm = (r >> 24) & 15, (r >> 15) & 511
        if ln["family"] != E.FAMILY_OF_KERNEL[kern]:
            bad.append(("family", ln["family"]))
        if kern in (E.IK["REG"], E.IK["DMA"], E.IK["P8"], E.IK["HALO"]) and ln["mtiles"] != -(-ln["m"] // bm):
            bad.append(("mtiles", ln["mtiles"], ln["m"], bm))
    elif case.method == "conv_wgrad":
        if (ln["route"], ln["ws"]) != (want["route"], want["ws"]):
            bad.append(("route", E.route_name(ln["route"]), ln["ws"], E.route_name(want["route"]), want["ws"]))
        if "splits" in want and ln["splits"] != want["splits"]:
            bad.append(("splits", ln["splits"], want["splits"]))
        if want.get("many") is not None and (ln["splits"] > 1) != want["many"]:
            bad.append(("many", ln["splits"]))
    for b in ln.get("bound", ()):
        if b["nparts"] is not None:
            bn_parts = TABLES[table].get("SFK_BN_PARTS", 1024)
            rule = nparts_rule(b["cgs"], b["pixels"], b["max_parts"] or 0, bn_parts)
            if b["nparts"] != rule:
                bad.append(("nparts", b, rule))
    return bad


def route_name(r: int) -> str:
    """conv_edges.route_name, with the two route bits of the tuned instantiations and the routes of the tuned lists spelt out"""
    base = r & ~(COGROUPS4 | RING5)
    name = E.route_name(base)
    if name.startswith("0x") and (base >> 24) & 15 == E.IK["P8"]:
        name = f"P8_T{(base >> 28) & 1}_{(base >> 15) & 511}x{(base >> 5) & 1023}_E{(base >> 2) & 7}_S{(base >> 1) & 1}_W{base & 1}"
    return name + ("_C1" if r & COGROUPS4 else "") + ("_R1" if r & RING5 else "")


def moved(table: str) -> List[str]:
    return sorted(set(MOVED_CONV[table]) | set(MOVED_WGRAD[table]) | set(MOVED_STEM[table]))
