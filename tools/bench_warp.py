#!/usr/bin/env python
"""The random affine augmentation on one GPU (include/sfk_warp.h): what sampling through a matrix costs beside shifting.

  kernel  at res3d.yaml's clip (N 30, T 20, 21 channels, S 192) and slowfast-HTAH.yaml's (N 55), f32 and bf16, from a pool of
          N*T distinct frames:
            1. sfk_u8_pool_gather_crop, the shipped kernel, untouched: the yardstick;
            2. sfk_u8_pool_gather_warp with integer-translation rows (the same clip, bit for bit -- asserted);
            3. sfk_u8_pool_gather_warp with draw_affine at the config defaults (degrees 10, scale (0.85, 1.15));
            4. F.grid_sample on the float clip of (1), with the second clip it allocates.
          One process; 3 warm-ups, then the variants alternate; every launch timed on its own with device events; median
          [min, max] of --launches.  Box-to-box spread is large: only the ratios within one process count.
  step    a host-fed eager bf16 train step (uint8 batch, pinned H2D, DevicePreprocess, TrainStep) at one geometry with
          MODEL.AFFINE off or on: run it once per setting, each in a fresh process.

One JSON line per row (kept in profiles/warp_bench.jsonl).
usage: python tools/bench_warp.py kernel [--launches 60] [--warmup 3] [--out FILE]
       python tools/bench_warp.py step --geometry res3d|htah --affine 0|1 [--reps 4] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda"
HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s
GEOMETRIES = {"res3d": ("res3d", 30), "htah": ("slowfast-HTAH", 55)}      # config -> (MODEL.NAME, batch size); T 20, S 192
ROWS = []


def emit(row):
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def bench_kernel(launches, warmup, t=20, c=21, s=192):
    import torch.nn.functional as F
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import draw_affine, draw_crop_offsets, normalize_lut
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    lut, pad = normalize_lut().to(DEV), s // 10
    for name, (_, n) in GEOMETRIES.items():
        g = torch.Generator().manual_seed(n)
        pool = torch.randint(0, 256, (n * t, s, s, c), generator=g, dtype=torch.uint8).to(DEV)
        index = torch.randperm(n * t, generator=g).to(torch.int32).view(n, t).to(DEV)
        crop = draw_crop_offsets(n, pad, g)
        shift = torch.tensor([[1.0, 0.0, l - pad, 0.0, 1.0, tp - pad] for tp, l in crop.tolist()])
        drawn = draw_affine(n, s, pad, 10.0, (0.85, 1.15), generator=g)
        fallback = sum(be.warp_fallback_tiles(s, s, c, c, r.tolist()) for r in drawn)
        crop_d, shift_d, drawn_d = crop.to(DEV), shift.to(DEV), drawn.to(DEV)
        # grid_sample's grid of the drawn rows: (n, s, s, 2) in [-1, 1], align_corners=False
        ar = torch.arange(s, dtype=torch.float32, device=DEV)
        k = [drawn_d[:, i][:, None, None] for i in range(6)]
        xs, ys = k[0] * ar[None, None, :] + k[1] * ar[None, :, None] + k[2], k[3] * ar[None, None, :] + k[4] * ar[None, :, None] + k[5]
        grid32 = torch.stack([(2 * xs + 1) / s - 1, (2 * ys + 1) / s - 1], -1)
        for dt in (torch.float32, torch.bfloat16):
            out = torch.empty(n, t, c, s, s, dtype=dt, device=DEV)
            ref = torch.empty_like(out)
            grid = grid32.to(dt)
            runs = {
                "sfk_u8_pool_gather_crop": be.u8_pool_gather_crop(pool, index, lut, 127, crop_d, pad, ref),
                "sfk_u8_pool_gather_warp integer translation": be.u8_pool_gather_warp(pool, index, lut, 127, shift_d, out),
                "sfk_u8_pool_gather_warp draw_affine defaults": be.u8_pool_gather_warp(pool, index, lut, 127, drawn_d, out),
            }
            variants = {k_: (lambda r=r: r(st)) for k_, r in runs.items()}
            variants["F.grid_sample on the float clip"] = lambda: F.grid_sample(ref.view(n, t * c, s, s), grid, mode="bilinear",
                                                                                padding_mode="zeros", align_corners=False)
            runs["sfk_u8_pool_gather_crop"](st)
            runs["sfk_u8_pool_gather_warp integer translation"](st)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), "integer-translation rows must reproduce the crop gather bit for bit"
            try:
                variants["F.grid_sample on the float clip"]()
            except RuntimeError as e:           # a dtype this torch build's grid_sample does not take: say so, time the rest
                emit({"bench": "warp_kernel", "geometry": name, "variant": "F.grid_sample on the float clip",
                      "dtype": str(dt).split(".")[1], "not_measured": str(e).splitlines()[0][:120]})
                del variants["F.grid_sample on the float clip"]
            for _ in range(warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            extra = 0
            if "F.grid_sample on the float clip" in variants:
                base_mem = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                variants["F.grid_sample on the float clip"]()
                torch.cuda.synchronize()
                extra = torch.cuda.max_memory_allocated() - base_mem
            ms = {k_: [] for k_ in variants}
            for _ in range(launches):
                for k_, fn in variants.items():
                    ms[k_].append(_timed(fn))
            base = statistics.median(ms["sfk_u8_pool_gather_crop"])
            written, read = out.numel() * out.element_size(), n * t * s * s * c
            for k_ in variants:
                med = statistics.median(ms[k_])
                emit({"bench": "warp_kernel", "geometry": name, "variant": k_, "shape": [n, t, c, s, s], "dtype": str(dt).split(".")[1],
                      "launches": launches, **_spread(ms[k_]), "vs_crop": round(med / base, 3), "bytes_written": written,
                      "frame_bytes": read, "hbm_fraction": round((written + read) / (med * 1e-3) / HBM_PEAK, 3),
                      "extra_bytes": int(extra) if k_.startswith("F.grid_sample") else 0,
                      "fallback_tiles": fallback if "draw_affine" in k_ else 0})
            del out, ref, grid
        del pool


def bench_step(geometry, affine, reps, rounds):
    from torch.utils.data.dataloader import default_collate
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer
    name, n = GEOMETRIES[geometry]
    with tempfile.TemporaryDirectory() as root:
        cfg = get_cfg()
        cfg.CHALEARN.ROOT = root
        cfg.MODEL.DTYPE = "bf16"
        cfg.MODEL.AFFINE = bool(affine)
        cfg.NUM_CPU = 0
        cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = n, 20
        cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT = name, "CropHTAH"
        tr = SyntheticChalearn(cfg, "train", num_videos=n, seed=1, as_uint8=True, frames_per_video=(20, 40))
        te = SyntheticChalearn(cfg, "test", num_videos=1, seed=2, frames_per_video=(20, 20))
        t = Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        t.model.train()
        host = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in default_collate([tr[i] for i in range(n)]).items()}
        assert ("warp" in host) == bool(affine) and ("crop" in host) != bool(affine)

        def run(k):
            for _ in range(k):
                x, y = t.mm.prepare_data(host)
                if isinstance(x, torch.Tensor):
                    t.step(x, None, y)
                else:
                    t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)
            torch.cuda.synchronize()
        run(2)
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            run(reps)
            ms.append((time.perf_counter() - t0) / reps * 1e3)
        emit({"bench": "warp_step", "geometry": geometry, "model": name, "dtype": "bf16", "clip": [n, 20, 21, 192, 192],
              "affine": bool(affine), "reps": reps, "rounds": rounds, "step": _spread(ms),
              "clip_launch": "sfk_u8_pool_gather_warp" if affine else "sfk_u8_normalize_crop"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--geometry", choices=sorted(GEOMETRIES), default="htah")
    ap.add_argument("--affine", type=int, choices=[0, 1], default=0)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warp.py measures on a GPU; there is no CPU path"
    if a.what == "kernel":
        bench_kernel(a.launches, a.warmup)
    else:
        bench_step(a.geometry, a.affine, a.reps, a.rounds)
    if a.out:
        with open(a.out, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")
