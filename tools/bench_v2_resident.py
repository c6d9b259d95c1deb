#!/usr/bin/env python
"""The device-resident v2 train set on one GPU (include/sfk_roi_pool.h, input_pipeline.ResidentGestureSet): what it costs and saves.

  kernel  sfk_roi_resize_pool (frames picked from a pool by index) against sfk_roi_resize writing the SAME output from the same
          frames stacked clip by clip: 10 clips x 20 frames of 240 x 320 x 7 to 192^2, antialias on, f32 and bf16, random part
          boxes.  Same process, alternating rounds after a warm-up, device events around `reps` launches a round; reported: the
          median and the [min, max] of the rounds' per-launch times.  The two read the same bytes.
  step    one bf16 train step of the v2 trainer (SlowFast depth 50, 10 x 20 x 7 x 192^2) fed two ways by the same Trainer,
          alternating: from a {'frames_u8', 'box'} batch that waits, already collated, in pinned host memory (H2D of 107 MB +
          RoiResize) and from the resident set (the tables' H2D + one sfk_roi_resize_pool launch; the frames were uploaded in
          the warm-up epochs).  Host clock around `reps` steps ending in a synchronise.  This prices the upload and nothing
          else: the frames are synthetic, so the DECODE a resident epoch saves (five decord readers per clip) and the host-side
          stacking and pinning of the loader are NOT in either number.

usage: python tools/bench_v2_resident.py [kernel|step ...] [--reps R] [--rounds K] [--out profiles/v2_resident_bench.jsonl]"""
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


def bench_kernel(reps, rounds, n=10, t=20, h=240, w=320, p=7, s=192, frames=40):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import byte_lut
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (n * frames, h, w, p), dtype=torch.uint8, device=DEV)      # n videos of `frames` frames
    start = torch.randint(0, frames - t + 1, (n,), generator=g)
    idx = (torch.arange(n)[:, None] * frames + start[:, None] + torch.arange(t)[None, :]).to(torch.int32)
    x1, y1 = torch.randint(0, w // 3, (n,), generator=g), torch.randint(0, h // 3, (n,), generator=g)
    x2, y2 = torch.randint(2 * w // 3, w + 1, (n,), generator=g), torch.randint(2 * h // 3, h + 1, (n,), generator=g)
    box = torch.stack([x1, y1, x2, y2], 1).to(torch.int32)
    idx_d, box_d, lut = idx.to(DEV), box.to(DEV), byte_lut().to(DEV)
    stacked = pool[idx_d.long()].contiguous()                                # (n, t, h, w, p): what a uint8 batch uploads
    box_bytes = int(((x2 - x1) * (y2 - y1)).sum()) * t * p
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(n, t, p, s, s, dtype=dt, device=DEV)
        ref = torch.empty_like(out)
        run_p = be.roi_resize_pool(pool, idx_d, lut, 127, box_d, out, True)
        run_s = be.roi_resize(stacked, lut, box_d, ref, True)
        for _ in range(3):
            run_s(st), run_p(st)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        ms_s, ms_p = [], []
        for _ in range(rounds):
            ms_s.append(_events(lambda: run_s(st), reps))
            ms_p.append(_events(lambda: run_p(st), reps))
        ob = out.numel() * out.element_size()
        emit({"bench": "roi_resize_pool_kernel", "shape": [n, t, p, s, s], "frame": [h, w, p], "antialias": True,
              "out_dtype": str(dt).split(".")[1], "out_bytes": ob, "u8_box_bytes": box_bytes, "u8_pool_bytes": pool.numel(),
              "reps": reps, "rounds": rounds, "roi_resize": _spread(ms_s), "roi_resize_pool": _spread(ms_p),
              "roi_resize_pool_gb_per_s": round((ob + box_bytes) / statistics.median(ms_p) / 1e6, 1)})


def bench_step(reps, rounds, n=10, t=20, s=192):
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd.config import get_cfg
    with tempfile.TemporaryDirectory() as root:
        cfg = get_cfg()
        cfg.CHALEARN.ROOT = root
        cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = n, t
        cfg.MODEL.NAME, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DTYPE = "gesture-v2", s, "bf16"
        cfg.MODEL.RESIDENT_TRAIN = True
        cfg.MODEL.RESIDENT_GB = 1.0
        cfg.NUM_CPU = 0
        tr = v2.SyntheticGesture(cfg, "train", num_videos=n, seed=1, videos=True, frames_per_video=(t, 2 * t))
        te = v2.SyntheticGesture(cfg, "test", num_videos=1, clips_per_video=(1, 1), seed=2)
        tnr = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        tnr.model.train()
        from torch.utils.data.dataloader import default_collate
        host = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in default_collate([tr[i] for i in range(n)]).items()}

        def step(batch):
            x, y = tnr.mm.prepare_data(batch)
            tnr.step(x[0], x[1], y, slow_t_index=tnr.model.slow_t_index)

        def fed(k):
            for _ in range(k):
                step(host)
            torch.cuda.synchronize()

        def resident(k, e0):
            for e in range(e0, e0 + k):
                for batch in tnr.resident.epoch(e):
                    step(batch)
            torch.cuda.synchronize()

        fed(2)
        resident(2, 0)                                                        # epoch 0 uploads every video, once
        uploaded = tnr.resident.bytes_uploaded
        ms_f, ms_r, e = [], [], 2
        for _ in range(rounds):
            t0 = time.perf_counter()
            fed(reps)
            ms_f.append((time.perf_counter() - t0) / reps * 1e3)
            t0 = time.perf_counter()
            resident(reps, e)
            ms_r.append((time.perf_counter() - t0) / reps * 1e3)
            e += reps
        assert tnr.resident.bytes_uploaded == uploaded and tnr.resident.spilled_clips == 0
        emit({"bench": "v2_resident_step", "dtype": "bf16", "clip": [n, t, 7, s, s], "frame": [tr.h, tr.w, 7], "reps": reps,
              "rounds": rounds, "first_timed_epoch": 2, "host_fed_u8_step": _spread(ms_f), "resident_step": _spread(ms_r),
              "h2d_bytes_per_host_fed_step": int(host["frames_u8"].numel()), "h2d_bytes_per_resident_step": n * t * 4 + n * 4 * 4,
              "resident_frames": tnr.resident.resident_frames, "resident_bytes_uploaded_once": int(uploaded),
              "note": "synthetic frames: the decode and the loader's stacking and pinning are in neither number"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "step"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_v2_resident.py measures on a GPU; there is no CPU path"
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
