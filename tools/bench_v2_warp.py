#!/usr/bin/env python
"""The random affine augmentation of the v2 part-box trainer on one GPU (include/sfk_roi_warp.h): what it costs.

  kernel  sfk_roi_resize_warp / _pool_warp / _ragged_warp with `draw_affine` rows at the config's default ranges against the
          sibling launch (sfk_roi_resize / _pool / _ragged with a RandomCrop row) reading the same frames: 10 clips x 20 frames
          of 240 x 320 x 7 to 192^2, antialias on and off, f32 and bf16, random part boxes.  Same process, alternating rounds
          after a warm-up, device events around `reps` launches a round; reported: the median and the [min, max] of the rounds'
          per-launch times.
  torch   the same clips by F.interpolate (the resize, written once) followed by F.grid_sample(bilinear, zeros,
          align_corners=False) (the sampling, a second float clip and a second interpolation) on the device, from the float
          box crops; its values differ from the kernel's (two interpolations), only the time is compared.
  step    one bf16 train step of the v2 trainer (SlowFast depth 50, 10 x 20 x 7 x 192^2) from a {'frames_u8', 'box'} batch that
          waits, already collated, in pinned host memory, with and without a 'warp' entry, alternating.  Host clock around
          `reps` steps ending in a synchronise.

usage: python tools/bench_v2_warp.py [kernel|torch|step ...] [--reps R] [--rounds K] [--out profiles/v2_warp_bench.jsonl]"""
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
DEFAULTS = (10.0, (0.85, 1.15), 0.0, 0.0)                      # MODEL.AFFINE_DEGREES, _SCALE, _SHEAR, _FLIP


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


def _geometry(n, t, h, w, p, frames, s):
    from video_classification_amd.input_pipeline import draw_affine, draw_crop_offsets
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (n * frames, h, w, p), dtype=torch.uint8, device=DEV)
    start = torch.randint(0, frames - t + 1, (n,), generator=g)
    idx = (torch.arange(n)[:, None] * frames + start[:, None] + torch.arange(t)[None, :]).to(torch.int32)
    x1, y1 = torch.randint(0, w // 3, (n,), generator=g), torch.randint(0, h // 3, (n,), generator=g)
    x2, y2 = torch.randint(2 * w // 3, w + 1, (n,), generator=g), torch.randint(2 * h // 3, h + 1, (n,), generator=g)
    box = torch.stack([x1, y1, x2, y2], 1).to(torch.int32)
    warp = draw_affine(n, s, s // 10, *DEFAULTS, generator=g)
    crop = draw_crop_offsets(n, s // 10, g)
    return pool, idx, box, warp, crop


def bench_kernel(reps, rounds, n=10, t=20, h=240, w=320, p=7, s=192, frames=40):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import byte_lut
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    pool, idx, box, warp, crop = _geometry(n, t, h, w, p, frames, s)
    idx_d, box_d, warp_d, crop_d, lut = idx.to(DEV), box.to(DEV), warp.to(DEV), crop.to(DEV), byte_lut().to(DEV)
    stacked = pool[idx_d.long()].contiguous()
    # the arena: every clip's frames cropped to its own box, packed
    parts, offs, at = [], [], 0
    for i in range(n):
        x1, y1, x2, y2 = box[i].tolist()
        fr = stacked[i, :, y1:y2, x1:x2].contiguous()
        at = -(-at // 16) * 16
        offs.append([at + k * fr[0].numel() for k in range(t)])
        parts.append((at, fr.view(-1)))
        at += fr.numel()
    arena = torch.zeros(-(-at // 16) * 16, dtype=torch.uint8, device=DEV)
    for o, b in parts:
        arena[o:o + b.numel()] = b
    off_d = torch.tensor(offs, dtype=torch.int64).to(DEV)
    hw = torch.stack([box[:, 3] - box[:, 1], box[:, 2] - box[:, 0]], 1).to(torch.int32)
    rbox = torch.stack([torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), hw[:, 1], hw[:, 0]], 1).contiguous()
    hw_d, rbox_d, max_hw = hw.to(DEV), rbox.to(DEV), (int(hw[:, 0].max()), int(hw[:, 1].max()))
    for aa in (True, False):
        for dt in (torch.float32, torch.bfloat16):
            out = torch.empty(n, t, p, s, s, dtype=dt, device=DEV)
            ref = torch.empty_like(out)
            pairs = {
                "stacked": (be.roi_resize(stacked, lut, box_d, ref, aa, crop_d, s // 10),
                            be.roi_resize_warp(stacked, lut, box_d, warp_d, out, aa)),
                "pool": (be.roi_resize_pool(pool, idx_d, lut, 127, box_d, ref, aa, crop_d, s // 10),
                         be.roi_resize_pool_warp(pool, idx_d, lut, 127, box_d, warp_d, out, aa)),
                "ragged": (be.roi_resize_ragged(arena, off_d, hw_d, lut, 127, rbox_d, ref, aa, crop_d, s // 10, pitch=p, max_hw=max_hw),
                           be.roi_resize_ragged_warp(arena, off_d, hw_d, lut, 127, rbox_d, warp_d, out, aa, pitch=p, max_hw=max_hw)),
            }
            for src, (run_c, run_w) in pairs.items():
                for _ in range(3):
                    run_c(st), run_w(st)
                torch.cuda.synchronize()
                ms_c, ms_w = [], []
                for _ in range(rounds):
                    ms_c.append(_events(lambda: run_c(st), reps))
                    ms_w.append(_events(lambda: run_w(st), reps))
                ob = out.numel() * out.element_size()
                emit({"bench": "roi_warp_kernel", "source": src, "shape": [n, t, p, s, s], "frame": [h, w, p], "antialias": aa,
                      "out_dtype": str(dt).split(".")[1], "out_bytes": ob, "affine": list(DEFAULTS[:1]) + [list(DEFAULTS[1])] + list(DEFAULTS[2:]),
                      "reps": reps, "rounds": rounds, "sibling_with_crop": _spread(ms_c), "warp": _spread(ms_w),
                      "ratio": round(statistics.median(ms_w) / statistics.median(ms_c), 3)})


def bench_torch(reps, rounds, n=10, t=20, h=240, w=320, p=7, s=192, frames=40):
    import torch.nn.functional as F
    pool, idx, box, warp, _ = _geometry(n, t, h, w, p, frames, s)
    stacked = pool[idx.to(DEV).long()]
    crops = []
    for i in range(n):
        x1, y1, x2, y2 = box[i].tolist()
        crops.append(stacked[i, :, y1:y2, x1:x2].permute(0, 3, 1, 2).float().div(255).contiguous())      # t p bh bw
    m = warp.to(DEV).view(n, 2, 3)
    ys, xs = torch.meshgrid(torch.arange(s, device=DEV, dtype=torch.float32), torch.arange(s, device=DEV, dtype=torch.float32), indexing="ij")
    u = m[:, 0, 0, None, None] * xs + m[:, 0, 1, None, None] * ys + m[:, 0, 2, None, None]
    v = m[:, 1, 0, None, None] * xs + m[:, 1, 1, None, None] * ys + m[:, 1, 2, None, None]
    grid = torch.stack([(2 * u + 1) / s - 1, (2 * v + 1) / s - 1], -1)                                     # n s s 2
    for aa in (True, False):
        def run():
            outs = []
            for i in range(n):
                r = F.interpolate(crops[i], (s, s), mode="bilinear", align_corners=False, antialias=aa)
                outs.append(F.grid_sample(r, grid[i:i + 1].expand(t, s, s, 2), mode="bilinear", padding_mode="zeros", align_corners=False))
            return torch.stack(outs)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = [_events(run, max(reps // 2, 1)) for _ in range(rounds)]
        emit({"bench": "roi_warp_torch", "shape": [n, t, p, s, s], "frame": [h, w, p], "antialias": aa, "out_dtype": "float32",
              "reps": max(reps // 2, 1), "rounds": rounds, "interpolate_then_grid_sample": _spread(ms),
              "note": "from float box crops already on the device; the uint8 -> float conversion is not timed"})


def bench_step(reps, rounds, n=10, t=20, s=192):
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd.config import get_cfg
    from video_classification_amd.input_pipeline import draw_affine
    with tempfile.TemporaryDirectory() as root:
        cfg = get_cfg()
        cfg.CHALEARN.ROOT = root
        cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = n, t
        cfg.MODEL.NAME, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DTYPE = "gesture-v2", s, "bf16"
        cfg.NUM_CPU = 0
        tr = v2.SyntheticGesture(cfg, "train", num_videos=n, seed=1)
        te = v2.SyntheticGesture(cfg, "test", num_videos=1, clips_per_video=(1, 1), seed=2)
        tnr = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        tnr.model.train()
        from torch.utils.data.dataloader import default_collate
        host = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in default_collate([tr[i] for i in range(n)]).items()}
        warped = dict(host, warp=draw_affine(n, s, s // 10, *DEFAULTS, generator=torch.Generator().manual_seed(3)))

        def fed(batch, k):
            for _ in range(k):
                x, y = tnr.mm.prepare_data(batch)
                tnr.step(x[0], x[1], y, slow_t_index=tnr.model.slow_t_index)
            torch.cuda.synchronize()

        fed(host, 2), fed(warped, 2)
        ms_off, ms_on = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            fed(host, reps)
            ms_off.append((time.perf_counter() - t0) / reps * 1e3)
            t0 = time.perf_counter()
            fed(warped, reps)
            ms_on.append((time.perf_counter() - t0) / reps * 1e3)
        emit({"bench": "v2_warp_step", "dtype": "bf16", "clip": [n, t, 7, s, s], "frame": [tr.h, tr.w, 7], "antialias": True,
              "reps": reps, "rounds": rounds, "host_fed_step_affine_off": _spread(ms_off), "host_fed_step_affine_on": _spread(ms_on),
              "ratio": round(statistics.median(ms_on) / statistics.median(ms_off), 4)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "torch", "step"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_v2_warp.py measures on a GPU; there is no CPU path"
    for w in a.what:
        if w == "kernel":
            bench_kernel(a.reps, a.rounds)
        elif w == "torch":
            bench_torch(a.reps, a.rounds)
        elif w == "step":
            bench_step(max(a.reps // 2, 2), a.rounds)
        else:
            raise SystemExit(f"unknown bench {w!r}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")
