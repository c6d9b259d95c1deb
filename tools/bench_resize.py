#!/usr/bin/env python
"""The raw transport on one GPU: what padding and resizing the v1 crops on the device (include/sfk_resize.h,
input_pipeline.PadResize) costs and saves.

  kernel  sfk_u8_pad_resize_cubic at the two ends of crop_resize_dict: 640 frames (a 32 x 20 batch) to 192 x 192 x 21 from
          sources around 240 x 200, and 640 frames to 64 x 64 x 21 from sources around 50 x 40.  Device events after warm-up;
          GB/s over the bytes it must move (raw bytes in, resized frames out).  Beside it, as a bytes-moved yardstick,
          sfk_u8_normalize_crop writing the float32 clip from the same number of resized frames.
  step    a bf16 SlowFast (depth 50) step at slowfast-HTAH.yaml's size with a 32 x 20 batch, fed from a pinned host batch
          every step as a loader feeds it: '<key>_u8' items (the frames already resized, as cv2_read_frame hands them over)
          against '<key>_raw' items (collate_raw's batch of the ragged crops).  ms/step including the H2D copies, PadResize
          and the step (wall clock, synchronised), and the bytes sent host to device per batch.  One mode per child process.
          The host's own cv2.resize time, which the raw items save, is NOT in either number.
  cv2     the maximum and mean absolute difference to cv2.resize(INTER_CUBIC) on random frames, when cv2 is importable;
          otherwise a row saying that it could not be measured.

usage: python tools/bench_resize.py [kernel|step|cv2 ...] [--steps K] [--warmup W]   (one JSON line per row)"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda"
FRAMES = 640
# target size: ((h lo, h hi), (w lo, w hi)) of the sources
ENDS = {192: ((200, 280), (160, 240)), 64: ((40, 60), (30, 50))}
MODES = ("u8", "raw")


def ragged_frames(f, size, seed, c=21):
    (hl, hh), (wl, wh) = ENDS[size]
    g = torch.Generator().manual_seed(seed)
    hs = torch.randint(hl, hh + 1, (f,), generator=g).tolist()
    ws = torch.randint(wl, wh + 1, (f,), generator=g).tolist()
    return [torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8) for h, w in zip(hs, ws)]


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


def bench_kernel(reps, warmup):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import normalize_lut, pack_raw_frames, raw_offsets
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    lut = normalize_lut().to(DEV)
    for size in ENDS:
        raw, hw = pack_raw_frames(ragged_frames(FRAMES, size, seed=size))
        offset = raw_offsets(hw, 21)
        out = torch.empty(FRAMES, size, size, 21, dtype=torch.uint8, device=DEV)
        op = be.u8_pad_resize_cubic(raw.to(DEV), offset.to(DEV), hw.to(DEV), out, size, int(hw.max()), 127)
        ms = _timed(lambda: op(st), reps, warmup)
        moved = raw.numel() + out.numel()
        clip = torch.empty(32, 20, 21, size, size, device=DEV)
        pre = be.u8_normalize_crop(out.view(32, 20, size, size, 21), lut, None, 0, clip)
        ms_pre = _timed(lambda: pre(st), reps, warmup)
        moved_pre = out.numel() + clip.numel() * 4
        print(json.dumps({"bench": "resize_kernel", "frames": FRAMES, "size": size, "mean_hw": [round(float(hw[:, 0].float().mean()), 1),
                                                                                          round(float(hw[:, 1].float().mean()), 1)],
                          "max_side": int(hw.max()), "raw_mb": round(raw.numel() / 1e6, 2), "out_mb": round(out.numel() / 1e6, 2),
                          "pad_resize_ms": round(ms, 4), "pad_resize_gb_s": round(moved / ms / 1e6, 1),
                          "normalize_crop_ms": round(ms_pre, 4), "normalize_crop_gb_s": round(moved_pre / ms_pre / 1e6, 1)}), flush=True)


def bench_step(mode, steps, warmup):
    from video_classification_amd.config import crop_resize_dict, get_cfg
    from video_classification_amd.input_pipeline import collate_raw, draw_crop_offsets, make_raw_item
    from video_classification_amd.train import ModelManager, TrainStep
    cfg = get_cfg()
    cfg.MODEL.DTYPE, cfg.MODEL.LR = "bf16", 1e-3
    cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT = "slowfast", "CropHTAH"
    cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.NUM_CLASS = 20, 32, 249
    n, t, key = 32, 20, "CropHTAH"
    s = crop_resize_dict[key]
    mm = ModelManager(cfg, DEV)
    m = mm.init_model()
    step = TrainStep(m.engine, lr=cfg.MODEL.LR, use_graph=False)
    g = torch.Generator().manual_seed(1)
    labels = torch.randint(0, 249, (n,), generator=g)
    batches = []
    for k in range(2):                                   # two pinned host batches alternate so every step copies a batch
        crop = draw_crop_offsets(n, s // 10, g)
        if mode == "u8":
            b = {key + "_u8": torch.randint(0, 256, (n, t, s, s, 21), generator=g, dtype=torch.uint8), "crop": crop, "label": labels}
        else:
            frames = ragged_frames(n * t, s, seed=10 + k)
            items = [dict(make_raw_item(key, frames[i * t:(i + 1) * t], int(labels[i])), crop=crop[i]) for i in range(n)]
            b = collate_raw(items)
        batches.append({k_: (v.pin_memory() if isinstance(v, torch.Tensor) else v) for k_, v in b.items()})

    def one(i):
        x, y = mm.prepare_data(batches[i % 2])
        step(x[0], x[1], y, slow_t_index=m.slow_t_index)

    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    sent = sum(v.numel() * v.element_size() for k_, v in batches[0].items() if k_ != "label")
    print(json.dumps({"bench": "resize_step", "mode": mode, "n": n, "t": t, "s": s, "ms_per_step": round(ms, 3),
                      "h2d_bytes_per_batch": int(sent), "steps": steps}), flush=True)


def bench_cv2():
    try:
        import cv2
    except Exception as e:
        print(json.dumps({"bench": "resize_cv2", "measured": False, "why": f"cv2 is not importable here ({type(e).__name__})"}), flush=True)
        return
    import numpy as np
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import PadResize, pack_raw_frames, raw_offsets
    for size in ENDS:
        frames = ragged_frames(40, size, seed=7)
        raw, hw = pack_raw_frames(frames)
        got = PadResize(size, DEV, HipBackend())(raw, raw_offsets(hw, 21), hw).cpu().numpy().astype(np.int64)
        worst, total, count = 0, 0, 0
        for i, f in enumerate(frames):
            h, w, c = f.shape
            m = max(h, w)
            sq = np.zeros((m, m, c), dtype=np.uint8)
            sq[(m - h) // 2:(m - h) // 2 + h, (m - w) // 2:(m - w) // 2 + w] = f.numpy()
            d = np.abs(got[i] - cv2.resize(sq, (size, size), interpolation=cv2.INTER_CUBIC).astype(np.int64))
            worst, total, count = max(worst, int(d.max())), total + int(d.sum()), count + d.size
        print(json.dumps({"bench": "resize_cv2", "measured": True, "size": size, "frames": len(frames), "max_abs_diff": worst,
                          "mean_abs_diff": round(total / count, 6)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "step", "cv2"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=MODES, help="step: this one mode in this process")
    a = ap.parse_args()
    for w in a.what:
        if w == "kernel":
            bench_kernel(a.steps, a.warmup)
        elif w == "step" and a.mode:
            bench_step(a.mode, a.steps, a.warmup)
        elif w == "step":
            for mode in MODES:       # a fresh process per mode (a failing child ends the run)
                subprocess.run([sys.executable, os.path.abspath(__file__), "step", "--mode", mode, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], check=True)
        elif w == "cv2":
            bench_cv2()
        else:
            raise SystemExit(f"unknown benchmark {w!r}")


if __name__ == "__main__":
    main()
