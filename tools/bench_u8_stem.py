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
  pool    MODEL.POOL_STEM's kernels (include/sfk_u8stem_pool.h): the u8 stems on the frames stacked clip by clip against the
          pooled u8 stems on the SAME frames lying in an arena behind a shuffled index table, forward + filter gradient (bf16),
          at the three sizes.  Same process, alternating rounds after a warm-up, device events around `--steps` passes a round;
          reported: the median and the [min, max] of the rounds' per-pass times.
  pool_step   one train step of slowfast-HTAH.yaml (bf16 SlowFast, depth 50, 55 x 20 x 21 x 192^2) fed by the resident set with
          MODEL.POOL_STEM off (one gather launch writes the float clip) and on (the stems read the arena): two Trainers in one
          process, alternating rounds of `--steps` steps, host clock ending in a synchronise.
  pool_mem    torch.cuda.max_memory_allocated over the timed steps of the same feed, each switch position in a fresh child
          process (so that the peak of one holds nothing of the other).

usage: python tools/bench_u8_stem.py [stems|res2d|htah|pool|pool_step|pool_mem ...] [--steps K] [--warmup W] [--rounds R]
       [--configs res2d.yaml,...] [--out profiles/pool_stem_bench.jsonl]      (one JSON line per row)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from video_classification_amd._lib import FMap, HipBackend, StemSrc, stem_kp
from video_classification_amd.input_pipeline import DevicePreprocess, PoolClip, U8Clip, draw_crop_offsets, normalize_lut

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


ROWS = []


def emit(row):
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def bench_pool_stems(reps, warmup, rounds, configs=None, frames_per_video=40):
    """the stacked-frame u8 stems against the pooled ones on the same frames: n videos of frames_per_video frames in the
    arena, clip i = a window of video i, the rows of the index table shuffled among the clips"""
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    lut = normalize_lut().to(DEV)
    for name, (n, t, s, stems, f2d) in CONFIGS.items():
        if configs and name not in configs:
            continue
        pad = s // 10
        arena = torch.randint(0, 256, (n * frames_per_video, s, s, 21), dtype=torch.uint8, device=DEV)
        start = torch.randint(0, frames_per_video - t + 1, (n,), generator=g)
        video = torch.randperm(n, generator=g)
        index = (video[:, None] * frames_per_video + start[:, None] + torch.arange(t)[None, :]).to(torch.int32).to(DEV)
        crop = draw_crop_offsets(n, pad, g).to(DEV)
        frames = arena[index.long()].contiguous()                           # (n, t, s, s, 21): what a uint8 batch uploads
        ops_u, ops_p, checks = [], [], []
        for c0, c, cout in stems:
            kt = t if f2d else 1
            t_out = 1 if f2d else t
            ho = (s - 1) // 2 + 1
            y_u = FMap(torch.empty(n * t_out * ho * ho * cout, dtype=torch.bfloat16, device=DEV), n, t_out, ho, ho, cout)
            y_p = FMap(torch.empty_like(y_u.buf), n, t_out, ho, ho, cout)
            kp = stem_kp(c, kt)
            w = torch.nn.functional.pad(torch.randn(cout, kt, c, 7, 7, generator=g) * 0.05, (0, 1)).reshape(cout, -1)
            w = torch.nn.functional.pad(w, (0, kp - w.shape[1])).reshape(-1).bfloat16().to(DEV)   # the stem layout
            dw = torch.zeros(cout * kp, device=DEV)
            su = StemSrc(U8Clip(frames, c0, c, crop, pad, lut), None, kt)
            sp = StemSrc(PoolClip(arena, index, c0, c, crop, pad, lut, 127), None, kt)
            stats = torch.empty(be.u8stem_tiles(su, y_u) * cout * 2, device=DEV)
            if f2d:
                ops_u += [be.u8stem2d_fwd(su, w, y_u, stats), be.u8stem2d_wgrad(su, y_u, dw)]
                ops_p += [be.u8pstem2d_fwd(sp, w, y_p, stats), be.u8pstem2d_wgrad(sp, y_p, dw)]
            else:
                ops_u += [be.u8stem_conv_fwd(su, w, y_u, stats), be.u8stem_conv_wgrad(su, y_u, dw)]
                ops_p += [be.u8pstem_conv_fwd(sp, w, y_p, stats), be.u8pstem_conv_wgrad(sp, y_p, dw)]
            checks.append((y_u, y_p))
        run_u, run_p = (lambda: [op(st) for op in ops_u]), (lambda: [op(st) for op in ops_p])
        for _ in range(warmup):
            run_u(), run_p()
        torch.cuda.synchronize()
        assert all(torch.equal(a.buf.view(torch.int16), b.buf.view(torch.int16)) for a, b in checks)
        ms_u, ms_p = [], []
        per_u, per_p = [[] for _ in ops_u], [[] for _ in ops_p]              # ... and launch by launch: (stem, fwd | wgrad)
        for _ in range(rounds):
            ms_u.append(_timed(run_u, reps, 0))
            ms_p.append(_timed(run_p, reps, 0))
            for i, (ou, op) in enumerate(zip(ops_u, ops_p)):
                per_u[i].append(_timed(lambda: ou(st), reps, 0))
                per_p[i].append(_timed(lambda: op(st), reps, 0))
        names = [f"c{c0}:{c0 + c}_{what}" for c0, c, _ in stems for what in ("fwd", "wgrad")]
        emit({"bench": "pool_stems", "config": name, "n": n, "t": t, "s": s, "pathways": len(stems), "dtype": "bf16",
              "u8_bytes_read": int(frames.numel()), "u8_pool_bytes": int(arena.numel()), "reps": reps, "rounds": rounds,
              "u8_stems_stacked": _spread(ms_u), "u8_stems_pooled": _spread(ms_p),
              "pooled_vs_stacked": round(statistics.median(ms_p) / statistics.median(ms_u), 4),
              "per_launch": {nm: {"stacked": _spread(u), "pooled": _spread(p)} for nm, u, p in zip(names, per_u, per_p)}})
        del arena, frames, ops_u, ops_p, checks
        torch.cuda.empty_cache()


def _resident_trainer(root, pool_stem):
    """bench_resident.py's slowfast-HTAH.yaml resident feed, with the switch"""
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = root
    cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = 55, 20
    cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT, cfg.MODEL.DTYPE = "slowfast-HTAH", "CropHTAH", "bf16"
    cfg.MODEL.RESIDENT_TRAIN, cfg.MODEL.RESIDENT_GB, cfg.MODEL.POOL_STEM = True, 4.0, bool(pool_stem)
    cfg.NUM_CPU = 0
    tr = SyntheticChalearn(cfg, "train", num_videos=55, seed=1, as_uint8=True, frames_per_video=(20, 40))
    te = SyntheticChalearn(cfg, "test", num_videos=1, seed=2, pooled=True, frames_per_video=(20, 20))
    torch.manual_seed(0)
    t = Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    t.model.train()
    return t


def _resident_steps(t, k, e0):
    for e in range(e0, e0 + k):
        for batch in t.resident.epoch(e):
            x, y = t.mm.prepare_data(batch)
            t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)
    torch.cuda.synchronize()


def bench_pool_step(reps, warmup, rounds):
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        ts = {"off": _resident_trainer(root, False), "on": _resident_trainer(root, True)}
        for t in ts.values():
            _resident_steps(t, max(warmup, 2), 0)                            # epoch 0 uploads every video, once
        ms, e = {"off": [], "on": []}, max(warmup, 2)
        for _ in range(rounds):
            for k, t in ts.items():
                t0 = time.perf_counter()
                _resident_steps(t, reps, e)
                ms[k].append((time.perf_counter() - t0) / reps * 1e3)
            e += reps
        assert all(t.resident.spilled_clips == 0 for t in ts.values())
        emit({"bench": "pool_stem_step", "config": "slowfast-HTAH.yaml", "dtype": "bf16", "clip": [55, 20, 21, 192, 192],
              "reps": reps, "rounds": rounds, "pool_stem_off_step": _spread(ms["off"]), "pool_stem_on_step": _spread(ms["on"]),
              "on_vs_off": round(statistics.median(ms["on"]) / statistics.median(ms["off"]), 4),
              "resident_frames": ts["on"].resident.resident_frames})


def bench_pool_mem(mode, steps, warmup):
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        t = _resident_trainer(root, mode == "on")
        _resident_steps(t, max(warmup, 2), 0)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        _resident_steps(t, steps, max(warmup, 2))
        ms = (time.perf_counter() - t0) / steps * 1e3
        emit({"bench": "pool_stem_mem", "config": "slowfast-HTAH.yaml", "dtype": "bf16", "pool_stem": mode, "steps": steps,
              "ms_per_step": round(ms, 3), "allocated_before_gb": round(base / 1e9, 3),
              "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3),
              "arena_gb": round(t.resident.pool.arena.numel() / 1e9, 3)})


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
    ap.add_argument("--mode", choices=MODES + ("off", "on"), help="res2d / htah / pool_mem: this one mode in this process")
    ap.add_argument("--rounds", type=int, default=5, help="pool / pool_step: alternating rounds")
    ap.add_argument("--out", default=None, help="pool / pool_step / pool_mem: append the rows to this file as well")
    a = ap.parse_args()
    for w in a.what:
        if w == "stems":
            bench_stems(a.steps, a.warmup, [c for c in a.configs.split(",") if c])
        elif w == "pool":
            bench_pool_stems(a.steps, a.warmup, a.rounds, [c for c in a.configs.split(",") if c])
        elif w == "pool_step":
            bench_pool_step(a.steps, a.warmup, a.rounds)
        elif w == "pool_mem" and a.mode:
            bench_pool_mem(a.mode, a.steps, a.warmup)
        elif w == "pool_mem":
            for mode in ("off", "on"):   # a fresh process per switch position (a failing child ends the run)
                subprocess.run([sys.executable, os.path.abspath(__file__), w, "--mode", mode, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)] + (["--out", a.out] if a.out else []), check=True)
        elif w in ("res2d", "htah") and a.mode:
            bench_host_fed(w, a.mode, a.steps, a.warmup)
        elif w in ("res2d", "htah"):
            for mode in MODES:       # a fresh process per mode (a failing child ends the run)
                subprocess.run([sys.executable, os.path.abspath(__file__), w, "--mode", mode, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], check=True)
        else:
            raise SystemExit(f"unknown benchmark {w!r}")
    if a.out and ROWS:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
