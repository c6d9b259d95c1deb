#!/usr/bin/env python
"""MODEL.U8_STEM on one GPU: what reading the uint8 frames inside the stems (include/sfk_u8stem.h) saves.

  stems   stem forward + filter gradient (bf16) with the batch already on the device, at the reference's res2d.yaml,
          res3d.yaml and slowfast-HTAH.yaml sizes (both SlowFast pathways): DevicePreprocess + the float-source stems,
          the float-source stems alone, and the u8 stems.  Device events after warm-up.
  res2d   a bf16 res2d engine step at res2d.yaml fed from a pinned host batch every step, as a loader feeds it: float32
          batch, uint8 batch with U8_STEM off (DevicePreprocess), uint8 with U8_STEM on.  ms/step including the H2D copy
          and the step (wall clock over the steps, synchronised), and torch.cuda.max_memory_allocated.
  htah    the same three ways for the reference SlowFast (depth 50) at slowfast-HTAH.yaml.
          Each of the three modes runs in a fresh child process with its own model, so the peak memory of one mode holds
          nothing of another (the engine's plan cache keeps each plan's last inputs alive).

usage: python tools/bench_u8_stem.py [stems|res2d|htah ...] [--steps K] [--warmup W] [--configs res2d.yaml,...]
       (one JSON line per row)"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from video_classification_amd._lib import FMap, HipBackend, StemSrc, stem_kp
from video_classification_amd.input_pipeline import DevicePreprocess, U8Clip, draw_crop_offsets, normalize_lut

DEV = "cuda"
# name: (N, T, S, [(c0, c, cout)] per stem, 2-D stem)
CONFIGS = {"res2d.yaml": (60, 10, 128, [(0, 5, 64)], True),
           "res3d.yaml": (30, 20, 192, [(0, 5, 64)], False),
           "slowfast-HTAH.yaml": (55, 20, 192, [(0, 5, 64), (5, 15, 8)], False)}


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_stems(reps, warmup, configs=None):
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    lut = normalize_lut().to(DEV)
    pre = DevicePreprocess(DEV, be)
    for name, (n, t, s, stems, f2d) in CONFIGS.items():
        if configs and name not in configs:
            continue
        pad = s // 10
        frames = torch.randint(0, 256, (n, t, s, s, 21), generator=g, dtype=torch.uint8).to(DEV)
        crop = draw_crop_offsets(n, pad, g).to(DEV)
        full = pre(frames, crop, pad)                                       # (n, t, 21, s, s) f32
        ops_f, ops_u = [], []
        for c0, c, cout in stems:
            kt = t if f2d else 1
            t_out = 1 if f2d else t
            ho = (s - 1) // 2 + 1
            y = FMap(torch.empty(n * t_out * ho * ho * cout, dtype=torch.bfloat16, device=DEV), n, t_out, ho, ho, cout)
            kp = stem_kp(c, kt)
            w = torch.nn.functional.pad(torch.randn(cout, kt, c, 7, 7, generator=g) * 0.05, (0, 1)).reshape(cout, -1)
            w = torch.nn.functional.pad(w, (0, kp - w.shape[1])).reshape(-1).bfloat16().to(DEV)   # the stem layout
            dw = torch.zeros(cout * kp, device=DEV)
            sf = StemSrc(full.permute(0, 2, 1, 3, 4)[:, c0:c0 + c], None, kt)
            su = StemSrc(U8Clip(frames, c0, c, crop, pad, lut), None, kt)
            stats = torch.empty(be.u8stem_tiles(su, y) * cout * 2, device=DEV)
            if f2d:
                ops_f += [be.stem2d_fwd(sf, w, y, stats), be.stem2d_wgrad(sf, y, dw)]
                ops_u += [be.u8stem2d_fwd(su, w, y, stats), be.u8stem2d_wgrad(su, y, dw)]
            else:
                ops_f += [be.stem_conv_fwd(sf, w, y, stats), be.stem_conv_wgrad(sf, y, dw)]
                ops_u += [be.u8stem_conv_fwd(su, w, y, stats), be.u8stem_conv_wgrad(su, y, dw)]
        out = torch.empty_like(full)
        pre_op = be.u8_normalize_crop(frames, lut, crop, pad, out)
        ms_pre = _timed(lambda: pre_op(st), reps, warmup)
        ms_f = _timed(lambda: [op(st) for op in ops_f], reps, warmup)
        ms_u = _timed(lambda: [op(st) for op in ops_u], reps, warmup)
        ms_pf = _timed(lambda: (pre_op(st), [op(st) for op in ops_f]), reps, warmup)
        print(json.dumps({"bench": "stems", "config": name, "n": n, "t": t, "s": s, "pathways": len(stems),
                          "preprocess_ms": round(ms_pre, 3), "float_stems_ms": round(ms_f, 3),
                          "preprocess_plus_float_stems_ms": round(ms_pf, 3), "u8_stems_ms": round(ms_u, 3),
                          "u8_vs_float_stems": round(ms_u / ms_f, 3), "u8_vs_preprocess_plus_float": round(ms_u / ms_pf, 3)}),
              flush=True)
        del full, out, ops_f, ops_u
        torch.cuda.empty_cache()


def _cfg(model):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DTYPE = "bf16"
    cfg.MODEL.LR = 1e-3
    if model == "res2d":
        cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT, cfg.MODEL.RES2D_BACKEND = "res2d", "CropLHandArm", "engine"
        cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.BATCH_SIZE = 10, 60
    else:
        cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT = "slowfast", "CropHTAH"
        cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.NUM_CLASS = 20, 55, 249
    return cfg


MODES = ("float32", "uint8", "uint8+U8_STEM")


def bench_host_fed(model, mode, steps, warmup):
    """one engine model, one input mode; two pinned host batches alternate so every step copies a batch"""
    from video_classification_amd.train import ModelManager, TrainStep
    cfg = _cfg(model)
    n, t = cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN
    from video_classification_amd.config import crop_resize_dict
    s = crop_resize_dict[cfg.MODEL.R3D_INPUT]
    key = cfg.MODEL.R3D_INPUT
    mm = ModelManager(cfg, DEV)
    m = mm.init_model()
    step = TrainStep(m.engine, lr=cfg.MODEL.LR, use_graph=False)
    g = torch.Generator().manual_seed(1)
    labels = torch.randint(0, 7, (n,), generator=g)
    u8s, crops = [], []
    for _ in range(2):
        u8s.append(torch.randint(0, 256, (n, t, s, s, 21), generator=g, dtype=torch.uint8).pin_memory())
        crops.append(draw_crop_offsets(n, s // 10, g).pin_memory())
    for mode in (mode,):
        cfg.MODEL.U8_STEM = mode == "uint8+U8_STEM"
        if mode == "float32":         # the loader's contiguous (N, T, 21, S, S) float32 batch
            batches = [{key: u.permute(0, 1, 4, 2, 3).contiguous().float().div_(255).sub_(0.45).div_(0.225).pin_memory(),
                        "label": labels} for u in u8s]
        else:
            batches = [{key + "_u8": u, "crop": c, "label": labels} for u, c in zip(u8s, crops)]

        def one(i):
            x, y = mm.prepare_data(batches[i % 2])
            if isinstance(x, (torch.Tensor, U8Clip)):
                step(x, None, y)
            else:
                step(x[0], x[1], y, slow_t_index=m.slow_t_index)

        for i in range(warmup):
            one(i)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for i in range(steps):
            one(i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        host_mb = sum(v.numel() * v.element_size() for k, v in batches[0].items() if k != "label") / 1e6
        print(json.dumps({"bench": model, "mode": mode, "n": n, "t": t, "s": s, "ms_per_step": round(ms, 3),
                          "host_batch_mb": round(host_mb, 1),
                          "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3)}), flush=True)
        del batches
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["stems", "res2d", "htah"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="", help="stems: comma-separated subset of " + ",".join(CONFIGS))
    ap.add_argument("--mode", choices=MODES, help="res2d / htah: this one mode in this process")
    a = ap.parse_args()
    for w in a.what:
        if w == "stems":
            bench_stems(a.steps, a.warmup, [c for c in a.configs.split(",") if c])
        elif w in ("res2d", "htah") and a.mode:
            bench_host_fed(w, a.mode, a.steps, a.warmup)
        elif w in ("res2d", "htah"):
            for mode in MODES:       # a fresh process per mode (a failing child ends the run)
                subprocess.run([sys.executable, os.path.abspath(__file__), w, "--mode", mode, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], check=True)
        else:
            raise SystemExit(f"unknown benchmark {w!r}")


if __name__ == "__main__":
    main()
