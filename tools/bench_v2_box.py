#!/usr/bin/env python
"""The box-cropped resident v2 train set on one GPU (include/sfk_roi_ragged.h, input_pipeline.BoxArena,
ResidentGestureSet(store='box')) against the whole-frame one (include/sfk_roi_pool.h, FramePool, store='frame').

  kernel  sfk_roi_resize_ragged reading every clip's frames from box-cropped storage (each clip's 20 frames cropped to its
          own box, packed in a byte arena at 16-byte-aligned offsets) against sfk_roi_resize_pool reading the SAME clips from
          whole frames: 10 clips x 20 frames of 240 x 320 x 7 to 192^2, antialias on, f32 and bf16, the random part boxes of
          tools/bench_v2_resident.py.  The outputs are compared with torch.equal first.  Same process, alternating rounds
          after a warm-up, device events around `reps` launches a round; reported: the median and the [min, max] of the
          rounds' per-launch times.  The two read the same window bytes.
  bytes   SyntheticGesture(videos=True) at 240 x 320: the arena bytes a resident video holds and the H2D bytes of an
          all-spilled step under either store, with the mean area fraction of the synthetic rectangles beside them (host only).
  step    one bf16 train step of the v2 trainer (SlowFast depth 50, 10 x 20 x 7 x 192^2) fed by an ALL-SPILLED resident set of
          either store, alternating: every step uploads its clips' distinct frames, whole or cropped to the clip's box, and
          gathers them with one launch.  The videos wait decoded in host memory, so the number prices the crop (a slice and a
          copy per clip, in the main process), the pinning, the upload and the gather; the decode is in neither.

usage: python tools/bench_v2_box.py [kernel|bytes|step ...] [--reps R] [--rounds K] [--out profiles/v2_box_bench.jsonl]"""
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
    hw = torch.stack([y2 - y1, x2 - x1], 1).to(torch.int32)
    span = [-(-t * int(a) * int(b) * p // 16) * 16 for a, b in hw.tolist()]
    base = [sum(span[:k]) for k in range(n)]
    arena = torch.empty(sum(span), dtype=torch.uint8, device=DEV)
    for k in range(n):                                                        # clip k: its t frames cropped to its own box
        blk = pool[idx[k].long().to(DEV), int(y1[k]):int(y2[k]), int(x1[k]):int(x2[k])].contiguous().view(-1)
        arena[base[k]:base[k] + blk.numel()].copy_(blk)
    offset = torch.tensor([[base[k] + f * int(hw[k, 0]) * int(hw[k, 1]) * p for f in range(t)] for k in range(n)], dtype=torch.int64)
    rbox = torch.stack([torch.zeros_like(x1), torch.zeros_like(y1), x2 - x1, y2 - y1], 1).to(torch.int32)
    max_hw = (int(hw[:, 0].max()), int(hw[:, 1].max()))
    idx_d, box_d, lut = idx.to(DEV), box.to(DEV), byte_lut().to(DEV)
    off_d, hw_d, rbox_d = offset.to(DEV), hw.to(DEV), rbox.to(DEV)
    box_bytes = int(((x2 - x1) * (y2 - y1)).sum()) * t * p
    for dt in (torch.float32, torch.bfloat16):
        out = torch.empty(n, t, p, s, s, dtype=dt, device=DEV)
        ref = torch.empty_like(out)
        run_r = be.roi_resize_ragged(arena, off_d, hw_d, lut, 127, rbox_d, out, True, pitch=p, max_hw=max_hw)
        run_p = be.roi_resize_pool(pool, idx_d, lut, 127, box_d, ref, True)
        out_f = torch.empty_like(out)                                         # the same launch told the whole frame's extent
        run_f = be.roi_resize_ragged(arena, off_d, hw_d, lut, 127, rbox_d, out_f, True, pitch=p, max_hw=(h, w))
        for _ in range(3):
            run_p(st), run_r(st), run_f(st)
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(out_f, ref)
        ms_p, ms_r, ms_f = [], [], []
        for _ in range(rounds):
            ms_p.append(_events(lambda: run_p(st), reps))
            ms_r.append(_events(lambda: run_r(st), reps))
            ms_f.append(_events(lambda: run_f(st), reps))
        ob = out.numel() * out.element_size()
        emit({"bench": "roi_resize_ragged_kernel", "shape": [n, t, p, s, s], "frame": [h, w, p], "max_hw": list(max_hw),
              "antialias": True, "out_dtype": str(dt).split(".")[1], "out_bytes": ob, "u8_box_bytes": box_bytes,
              "u8_arena_bytes": arena.numel(), "u8_pool_bytes": pool.numel(), "reps": reps, "rounds": rounds,
              "roi_resize_pool": _spread(ms_p), "roi_resize_ragged": _spread(ms_r),
              "roi_resize_ragged_max_hw_frame": _spread(ms_f),
              "ragged_over_pool": round(statistics.median(ms_r) / statistics.median(ms_p), 4),
              "roi_resize_ragged_gb_per_s": round((ob + box_bytes) / statistics.median(ms_r) / 1e6, 1)})


def _cfg(root, n, t, s):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = root
    cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = n, t
    cfg.MODEL.NAME, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DTYPE = "gesture-v2", s, "bf16"
    cfg.NUM_CPU = 0
    return cfg


class Decoded:
    """a train set whose videos wait decoded in host memory: video_item is an index and a copy"""

    def __init__(self, ds):
        self.ds = ds
        self.frames = [ds.video_item(i)["frames_pool"] for i in range(len(ds))]
        self.seq_len, self.label, self.frame_boxes, self.h, self.w = ds.seq_len, ds.label, ds.frame_boxes, ds.h, ds.w

    def __len__(self):
        return len(self.ds)

    def video_item(self, i, indices=None):
        f = self.frames[i] if indices is None else self.frames[i][list(indices)]
        return {"frames_pool": f, "windows": torch.arange(f.shape[0], dtype=torch.int32)[None]}


def _spill_only(ds, cfg, store, n, device, backend=None):
    """a resident set of that store whose resident region holds no video: every clip is spilled"""
    from video_classification_amd.input_pipeline import ResidentGestureSet
    h, w, t = ds.h, ds.w, int(cfg.CHALEARN.CLIP_LEN)
    if store == "box":
        return ResidentGestureSet(ds, cfg, device, backend, batch_size=n, seed=0, store="box",
                                  capacity_bytes=n * (t * h * w * 7 + 16) + 16)
    return ResidentGestureSet(ds, cfg, device, backend, batch_size=n, seed=0, capacity_frames=n * t + 1)


def bench_bytes(n=10, t=20, s=192, videos=40, epochs=4):
    """host only: the plan's own arithmetic on the synthetic part boxes"""
    from video_classification_amd import gesture_v2 as v2
    with tempfile.TemporaryDirectory() as root:
        cfg = _cfg(root, n, t, s)
        ds = v2.SyntheticGesture(cfg, "train", num_videos=videos, seed=1, videos=True, frames_per_video=(t, 2 * t))
        frame = ds.h * ds.w * 7
        rect, whole, vid_frac = 0, 0, []
        for v in range(videos):
            b = ds.frame_boxes(v)
            x1, y1 = max(0, int(b[:, 0].min())), max(0, int(b[:, 1].min()))
            x2, y2 = min(ds.w, int(b[:, 2].max())), min(ds.h, int(b[:, 3].max()))
            rect += ds.seq_len(v) * (y2 - y1) * (x2 - x1) * 7
            whole += ds.seq_len(v) * frame
            vid_frac.append((y2 - y1) * (x2 - x1) / (ds.h * ds.w))

        class NoFrames:                                                       # the plan reads boxes and lengths only
            h, w = ds.h, ds.w
            seq_len, label, frame_boxes = staticmethod(ds.seq_len), staticmethod(ds.label), staticmethod(ds.frame_boxes)

            def __len__(self):
                return len(ds)

            def video_item(self, i, indices=None):
                return {"frames_pool": torch.zeros(1, ds.h, ds.w, 7, dtype=torch.uint8), "windows": torch.zeros(1, 1, dtype=torch.int32)}
        r = _spill_only(NoFrames(), cfg, "box", n, "cpu", object())           # a plan launches nothing: no backend is called
        box_b, frame_b, clip_frac, steps = 0, 0, [], 0
        for e in range(epochs):
            for videos_, indices, box, _, _ in r.plan(e):
                steps += 1
                for k in range(len(videos_)):
                    d = len(set(indices[k].tolist()))
                    bx = box[k].tolist()
                    box_b += d * (bx[3] - bx[1]) * (bx[2] - bx[0]) * 7
                    frame_b += d * frame
                    clip_frac.append((bx[3] - bx[1]) * (bx[2] - bx[0]) / (ds.h * ds.w))
        emit({"bench": "v2_box_bytes", "set": f"SyntheticGesture(videos=True, {videos} videos of {t}..{2 * t} frames, {ds.h}x{ds.w}x7)",
              "clip": [n, t], "arena_bytes_per_resident_video": {"frame": round(whole / videos), "box": round(rect / videos)},
              "video_rect_mean_area_fraction": round(statistics.mean(vid_frac), 4),
              "h2d_bytes_per_all_spilled_step": {"frame": round(frame_b / steps), "box": round(box_b / steps)},
              "clip_box_mean_area_fraction": round(statistics.mean(clip_frac), 4), "steps": steps,
              "note": "the synthetic boxes are uniform draws per frame: the union over a video or a 20-frame clip is nearly the frame"})


def bench_step(reps, rounds, n=10, t=20, s=192):
    from video_classification_amd import gesture_v2 as v2
    with tempfile.TemporaryDirectory() as root:
        cfg = _cfg(root, n, t, s)
        tr = v2.SyntheticGesture(cfg, "train", num_videos=n, seed=1, videos=True, frames_per_video=(t, 2 * t))
        te = v2.SyntheticGesture(cfg, "test", num_videos=1, clips_per_video=(1, 1), seed=2)
        tnr = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        tnr.model.train()
        ds = Decoded(tr)
        sets = {store: _spill_only(ds, cfg, store, n, DEV) for store in ("frame", "box")}

        def run(store, k, e0):
            for e in range(e0, e0 + k):
                for batch in sets[store].epoch(e):                            # one batch an epoch: n videos, batch size n
                    x, y = tnr.mm.prepare_data(batch)
                    tnr.step(x[0], x[1], y, slow_t_index=tnr.model.slow_t_index)
            torch.cuda.synchronize()

        for store in sets:
            run(store, 2, 0)
        ms, e = {"frame": [], "box": []}, 2
        for _ in range(rounds):
            for store in ("frame", "box"):
                t0 = time.perf_counter()
                run(store, reps, e)
                ms[store].append((time.perf_counter() - t0) / reps * 1e3)
            e += reps
        up = {}
        for store, r in sets.items():
            assert r.resident_videos == 0 and r.spilled_clips == n
            up[store] = round(r.bytes_uploaded / (e * 1.0))
        emit({"bench": "v2_box_spilled_step", "dtype": "bf16", "clip": [n, t, 7, s, s], "frame": [tr.h, tr.w, 7], "reps": reps,
              "rounds": rounds, "first_timed_epoch": 2, "frame_store_step": _spread(ms["frame"]), "box_store_step": _spread(ms["box"]),
              "h2d_frame_bytes_per_step": up,
              "note": "all-spilled feed, videos decoded in host memory: crop, pinning, upload and gather are in the number; the decode is not"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "bytes", "step"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    for w in a.what:
        if w == "bytes":
            bench_bytes()
            continue
        assert torch.cuda.is_available(), "bench_v2_box.py measures kernel and step on a GPU; there is no CPU path"
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
