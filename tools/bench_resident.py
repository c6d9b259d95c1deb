#!/usr/bin/env python
"""The device-resident train set on one GPU (include/sfk_resident.h, input_pipeline.ResidentTrainSet): what it costs and saves.

  kernel  sfk_u8_pool_gather_crop (frames gathered from a pool by index, cropped) against sfk_u8_normalize_crop writing the SAME
          output from the same frames stacked clip by clip: 55 clips x 20 frames x 21 channels x 128^2, f32 and bf16, random
          crops.  Same process, alternating rounds after a warm-up, device events around `reps` launches a round; reported: the
          median and the [min, max] of the rounds' per-launch times.  The same launch without a crop table, and
          sfk_u8_pool_gather, are timed beside them: what the crop itself costs.
  step    one train step of slowfast-HTAH.yaml (bf16 SlowFast, depth 50, 55 x 20 x 21 x 192^2) fed two ways by the same Trainer,
          alternating: from a '<R3D_INPUT>_u8' batch that waits, already collated, in pinned host memory (H2D + DevicePreprocess)
          and from the resident set (the tables' H2D + one gather launch; the frames were uploaded in the warm-up epoch).  Host
          clock around `reps` steps ending in a synchronise.  This prices the upload and nothing else: the frames are synthetic,
          so the DECODE a resident epoch saves (the reference's cv2.imread calls) and the host-side stacking and pinning of
          the loader are NOT in either number.

usage: python tools/bench_resident.py [kernel|step ...] [--reps R] [--rounds K] [--out profiles/resident_bench.jsonl]"""
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
ROWS = []


def emit(row):
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_kernel(reps, rounds, n=55, t=20, s=128, p=21, frames=40):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import draw_crop_offsets, normalize_lut
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (n * frames, s, s, p), dtype=torch.uint8, device=DEV)      # n videos of `frames` frames
    start = torch.randint(0, frames - t + 1, (n,), generator=g)
    idx = (torch.arange(n)[:, None] * frames + start[:, None] + torch.arange(t)[None, :]).to(torch.int32)
    pad = s // 10
    crop = draw_crop_offsets(n, pad, g)
    idx_d, crop_d, lut = idx.to(DEV), crop.to(DEV), normalize_lut().to(DEV)
    stacked = pool[idx_d.long()].contiguous()                                # (n, t, s, s, p): what a uint8 batch uploads
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(n, t, p, s, s, dtype=dt, device=DEV)
        ref = torch.empty_like(out)
        run_g = be.u8_pool_gather_crop(pool, idx_d, lut, 127, crop_d, pad, out)
        run_n = be.u8_normalize_crop(stacked, lut, crop_d, pad, ref)
        for _ in range(3):
            run_n(st), run_g(st)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        run_g0 = be.u8_pool_gather_crop(pool, idx_d, lut, 127, None, pad, ref)    # what the crop costs: the same launch without
        run_p0 = be.u8_pool_gather(pool, idx_d, lut, 127, ref)                    # one, and sfk_u8_pool_gather (sfk_pool.h)
        run_g0(st), run_p0(st)
        torch.cuda.synchronize()
        ms_n, ms_g, ms_g0, ms_p0 = [], [], [], []
        for _ in range(rounds):
            ms_n.append(_events(lambda: run_n(st), reps))
            ms_g.append(_events(lambda: run_g(st), reps))
            ms_g0.append(_events(lambda: run_g0(st), reps))
            ms_p0.append(_events(lambda: run_p0(st), reps))
        ob = out.numel() * out.element_size()
        emit({"bench": "pool_gather_crop_kernel", "shape": [n, t, p, s, s], "out_dtype": str(dt).split(".")[1], "out_bytes": ob,
              "u8_bytes_read": stacked.numel(), "u8_pool_bytes": pool.numel(), "reps": reps, "rounds": rounds,
              "normalize_crop": _spread(ms_n), "pool_gather_crop": _spread(ms_g),
              "pool_gather_crop_without_crop": _spread(ms_g0), "pool_gather": _spread(ms_p0),
              "pool_gather_crop_gb_per_s": round((ob + stacked.numel()) / statistics.median(ms_g) / 1e6, 1)})


def bench_step(reps, rounds, config="slowfast-HTAH.yaml"):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer
    with tempfile.TemporaryDirectory() as root:
        cfg = get_cfg()                                                       # the yaml's geometry, as tools/bench_eval_pool.py
        cfg.CHALEARN.ROOT = root
        cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = 55, 20
        cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT, cfg.MODEL.DTYPE = "slowfast-HTAH", "CropHTAH", "bf16"
        cfg.MODEL.RESIDENT_TRAIN = True
        cfg.MODEL.RESIDENT_GB = 4.0
        cfg.NUM_CPU = 0
        key, n = cfg.MODEL.R3D_INPUT, cfg.CHALEARN.BATCH_SIZE
        tr = SyntheticChalearn(cfg, "train", num_videos=n, seed=1, as_uint8=True, frames_per_video=(20, 40))
        te = SyntheticChalearn(cfg, "test", num_videos=1, seed=2, pooled=True, frames_per_video=(20, 20))
        t = Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        t.model.train()
        from torch.utils.data.dataloader import default_collate
        host = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in default_collate([tr[i] for i in range(n)]).items()}

        def step(batch):
            x, y = t.mm.prepare_data(batch)
            t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)

        def fed(k):
            for _ in range(k):
                step(host)
            torch.cuda.synchronize()

        def resident(k, e0):
            for e in range(e0, e0 + k):
                for batch in t.resident.epoch(e):
                    step(batch)
            torch.cuda.synchronize()

        fed(2)
        resident(2, 0)                                                        # epoch 0 uploads every video, once
        uploaded = t.resident.bytes_uploaded
        ms_f, ms_r, e = [], [], 2
        for _ in range(rounds):
            t0 = time.perf_counter()
            fed(reps)
            ms_f.append((time.perf_counter() - t0) / reps * 1e3)
            t0 = time.perf_counter()
            resident(reps, e)
            ms_r.append((time.perf_counter() - t0) / reps * 1e3)
            e += reps
        assert t.resident.bytes_uploaded == uploaded and t.resident.spilled_clips == 0
        emit({"bench": "resident_step", "config": config, "dtype": "bf16", "clip": [n, 20, 21, 192, 192], "reps": reps,
              "rounds": rounds, "host_fed_u8_step": _spread(ms_f), "resident_step": _spread(ms_r),
              "h2d_bytes_per_host_fed_step": int(host[key + "_u8"].numel()), "h2d_bytes_per_resident_step": n * 20 * 4 + n * 2 * 4,
              "resident_frames": t.resident.resident_frames, "resident_bytes_uploaded_once": int(uploaded),
              "note": "synthetic frames: the decode and the loader's stacking and pinning are in neither number"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resident.py measures on a GPU; there is no CPU path"
    for w in a.what:
        if w == "kernel":
            bench_kernel(a.reps, a.rounds)
        elif w == "step":
            bench_step(max(a.reps // 2, 2), a.rounds)
        else:
            raise SystemExit(f"unknown bench {w!r}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")
