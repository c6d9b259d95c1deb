#!/usr/bin/env python
"""Pooled evaluation on one GPU: what uploading every test frame once (include/sfk_pool.h, input_pipeline.FramePool) saves.

  eval    Trainer.run_eval (bf16 SlowFast, depth 50) over synthetic test videos of 60 frames at CLIP_LEN 20 -- K = 10 uniform
          windows a video, 200 frames as clips against 60 pooled -- at slowfast-LHand.yaml (64^2, batch 300) and
          slowfast-HTAH.yaml (192^2, batch 55), three ways: float32 clip lists (the reference's items), uint8 clip lists
          (DevicePreprocess), pooled videos (FramePool).  The items are built before the clock starts, so a run is collate +
          pin + H2D + forward + aggregation.  Each mode runs in a fresh child process.  Reported: clips/s over the timed
          run_evals (wall clock, synchronised), the bytes handed to the device per run_eval, torch.cuda.max_memory_allocated.
  kernel  sfk_u8_pool_gather against sfk_u8_normalize_crop writing the SAME output (55 x 20 x 21 x 192^2 and 300 x 20 x 21 x 64^2,
          f32), device events after warm-up; run this one under `rocprofv3 --kernel-trace --stats -- python tools/bench_eval_pool.py
          kernel`, in a run of its own, for the per-kernel times.

usage: python tools/bench_eval_pool.py [eval|kernel ...] [--reps R] [--configs slowfast-LHand.yaml,...]   (one JSON line per row)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda"
MODES = ("float32", "u8list", "pooled")
# name: (MODEL.NAME, R3D_INPUT, BATCH_SIZE of the yaml, test videos)
CONFIGS = {"slowfast-LHand.yaml": ("slowfast-LHand", "CropLHand", 300, 60),
           "slowfast-HTAH.yaml": ("slowfast-HTAH", "CropHTAH", 55, 11)}
FRAMES, CLIP_LEN = 60, 20


class _Items(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _cfg(name, root):
    from video_classification_amd.config import get_cfg
    model, key, bs, _ = CONFIGS[name]
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = root
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = CLIP_LEN
    cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT, cfg.MODEL.DTYPE = model, key, "bf16"
    cfg.NUM_CPU = 0
    return cfg


def bench_eval(name, mode, reps):
    from video_classification_amd.input_pipeline import unpool_item
    from video_classification_amd.train import SyntheticChalearn, Trainer
    with tempfile.TemporaryDirectory() as root:
        cfg = _cfg(name, root)
        key, videos = cfg.MODEL.R3D_INPUT, CONFIGS[name][3]
        pooled = SyntheticChalearn(cfg, "test", num_videos=videos, seed=2, pooled=True, frames_per_video=(FRAMES, FRAMES))
        items = [pooled[i] for i in range(videos)]
        if mode != "pooled":
            items = [unpool_item(it) for it in items]
        if mode == "float32":
            items = [[{key: ((c[key + "_u8"].float() / 255.0 - 0.45) / 0.225).permute(0, 3, 1, 2).contiguous(), "label": c["label"]}
                      for c in it] for it in items]
        tr = SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
        loader = torch.utils.data.DataLoader(_Items(items), batch_size=cfg.CHALEARN.BATCH_SIZE, shuffle=False, collate_fn=lambda x: x)
        t = Trainer(cfg, train_set=tr, test_set=_Items(items), device=DEV)
        sent = [0]
        prepare = t.mm.prepare_data

        def counted(batch):
            sent[0] += sum(v.numel() * v.element_size() for k, v in batch.items() if k != "label" and v.device.type == "cpu")
            return prepare(batch)
        t.mm.prepare_data = counted
        t.run_eval(loader)                                                    # warm-up: plans, code objects, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        sent[0] = 0
        t0 = time.perf_counter()
        for _ in range(reps):
            res = t.run_eval(loader)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        h2d = sent[0] // reps
        if mode == "pooled":
            h2d += t.frame_pool.bytes_uploaded + sum(it["windows"].numel() * 4 for it in items)
        clips = sum(res["sv"])
        print(json.dumps({"bench": "eval_pool", "config": name, "mode": mode, "videos": videos, "clips": clips,
                          "s_per_run_eval": round(dt, 4), "clips_per_s": round(clips / dt, 1), "h2d_bytes": int(h2d),
                          "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3)}), flush=True)


def _timed(fn, reps, warmup=3):
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


def bench_kernel(name, reps):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.config import crop_resize_dict
    from video_classification_amd.input_pipeline import normalize_lut, uniform_windows
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    _, key, n, _ = CONFIGS[name]
    s = crop_resize_dict[key]
    nv = (n + 9) // 10
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (nv * FRAMES, s, s, 21), generator=g, dtype=torch.uint8)
    win = uniform_windows(FRAMES, CLIP_LEN)
    idx = torch.cat([win + v * FRAMES for v in range(nv)])[:n].contiguous()
    stacked = pool[idx.long()].to(DEV)                                        # (n, T, s, s, 21): what a uint8 clip list uploads
    pool_d, idx_d, lut = pool.to(DEV), idx.to(DEV), normalize_lut().to(DEV)
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(n, CLIP_LEN, 21, s, s, dtype=dt, device=DEV)
        ref = torch.empty_like(out)
        run_g = be.u8_pool_gather(pool_d, idx_d, lut, 127, out)
        run_n = be.u8_normalize_crop(stacked, lut, None, 0, ref)
        ms_n, ms_g = _timed(lambda: run_n(st), reps), _timed(lambda: run_g(st), reps)
        ms_n2, ms_g2 = _timed(lambda: run_n(st), reps), _timed(lambda: run_g(st), reps)
        assert torch.equal(out, ref)
        ob = out.numel() * out.element_size()
        print(json.dumps({"bench": "pool_gather_kernel", "config": name, "out_dtype": str(dt).split(".")[1], "out_bytes": ob,
                          "u8_read_bytes_normalize_crop": stacked.numel(), "u8_pool_bytes": pool.numel(),
                          "normalize_crop_ms": [round(ms_n, 4), round(ms_n2, 4)], "pool_gather_ms": [round(ms_g, 4), round(ms_g2, 4)],
                          "pool_gather_out_gb_per_s": round(ob / min(ms_g, ms_g2) / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["eval", "kernel"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--mode", choices=MODES, help="eval: this one mode of ONE config in this process")
    a = ap.parse_args()
    configs = [c for c in a.configs.split(",") if c]
    for w in a.what:
        if w == "kernel":
            for c in configs:
                bench_kernel(c, max(a.reps, 10))
        elif w == "eval" and a.mode:
            bench_eval(configs[0], a.mode, a.reps)
        elif w == "eval":
            for c in configs:
                for mode in MODES:   # a fresh process per mode (a failing child ends the run)
                    subprocess.run([sys.executable, os.path.abspath(__file__), "eval", "--mode", mode, "--configs", c,
                                    "--reps", str(a.reps)], check=True)
        else:
            raise SystemExit(f"unknown bench {w!r}")
