#!/usr/bin/env python
"""Mixup / CutMix and the soft-target loss on one GPU (include/sfk_mix.h): what they cost.

  kernel  sfk_clip_mix at the HTAH clip (N 55, T 20, 21 channels, S 192; f32 and bf16) with all-mixup rows and with all-CutMix
          rows (lam ~ Beta(1, 1)), against the fastest plain-torch statement of the same result on the same tensors:
          torch.lerp against the flipped clip for Mixup, torch.where under the box mask for CutMix.  Reported: the bytes the
          launch needs, computed from the rows (both members read once wherever either changes, every changed element written
          once), over its time, as a share of 8 TB/s; and the extra peak memory torch's form allocates.
  loss    sfk_softmax_ce_mix (mixed rows, eps 0.1) against sfk_softmax_ce at (55, 249).
  step    a host-fed bf16 train step at slowfast-HTAH.yaml's geometry and at the v2 geometry (N 10, T 20, S 192) with the
          MODEL.LABEL_SMOOTHING / MIXUP_ALPHA / CUTMIX_ALPHA keys off and on: the same Trainer and model, two TrainSteps.

One process; after a warm-up the variants alternate; kernels are timed launch by launch with device events, steps with a host
clock around `reps` steps ending in a synchronise; median [min, max].  One JSON line per row (kept in profiles/mix_bench.jsonl).
usage: python tools/bench_mix.py [kernel|loss|step_htah|step_v2 ...] [--launches 30] [--reps 4] [--rounds 5] [--out FILE]"""
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


def mix_bytes(rows, t, c, h, w, esize):
    """the bytes one sfk_clip_mix launch needs for these rows: per pair, both members read wherever either changes, every
    changed element written once"""
    total = 0
    for a, ra in enumerate(rows.tolist()):
        p = int(ra[0])
        if p <= a:
            continue
        rb = rows[p].tolist()
        area = lambda r: max(0, int(r[4]) - int(r[2])) * max(0, int(r[5]) - int(r[3]))
        inter = (max(0, min(ra[4], rb[4]) - max(ra[2], rb[2])) * max(0, min(ra[5], rb[5]) - max(ra[3], rb[3]))) if area(ra) and area(rb) else 0
        wa = h * w if ra[1] != 1 else area(ra)
        wb = h * w if rb[1] != 1 else area(rb)
        need = h * w if (ra[1] != 1 or rb[1] != 1) else area(ra) + area(rb) - int(inter)
        total += (2 * need + wa + wb) * t * c * esize
    return total


def bench_kernel(launches, warmup, n=55, t=20, c=21, s=192):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import draw_mix
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(n, t, c, s, s, device=DEV).to(dt)
        for case, kw in (("mixup", dict(mixup_alpha=0.8)), ("cutmix", dict(cutmix_alpha=1.0))):
            rows = draw_mix(n, s, s, generator=g, **kw)
            table = rows.to(DEV)
            run = be.clip_mix(x, table)
            lam = table[:, 1].view(n, 1, 1, 1, 1).to(dt)
            mask = torch.zeros(n, 1, 1, s, s, dtype=torch.bool, device=DEV)
            for i, r in enumerate(rows.tolist()):
                mask[i, :, :, int(r[2]):int(r[4]), int(r[3]):int(r[5])] = True
            if case == "mixup":
                ref = lambda: torch.lerp(x.flip(0), x, lam)                    # lam x + (1 - lam) flip(x), out of place
            else:
                ref = lambda: torch.where(mask, x.flip(0), x)
            for _ in range(warmup):
                run(st)
                ref()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ref()
            torch.cuda.synchronize()
            extra = torch.cuda.max_memory_allocated() - base
            ms_k, ms_t = [], []
            for _ in range(launches):
                ms_k.append(_timed(lambda: run(st)))
                ms_t.append(_timed(ref))
            nbytes = mix_bytes(rows, t, c, s, s, x.element_size())
            med = statistics.median(ms_k)
            emit({"bench": "clip_mix_kernel", "case": case, "shape": [n, t, c, s, s], "dtype": str(dt).split(".")[1],
                  "launches": launches, "sfk_clip_mix": _spread(ms_k), "torch": _spread(ms_t),
                  "torch_form": "lerp(flip(x), x, lam)" if case == "mixup" else "where(mask, flip(x), x)",
                  "bytes_needed": nbytes, "clip_bytes": x.numel() * x.element_size(), "gb_per_s": round(nbytes / med / 1e6, 1),
                  "hbm_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3), "torch_over_kernel": round(statistics.median(ms_t) / med, 2),
                  "torch_extra_peak_bytes": int(extra), "kernel_extra_bytes": 0})
            # torch moves at least the flipped copy on top of the blend: an in-place kernel that loses to it is broken
            assert case != "mixup" or med <= statistics.median(ms_t), (med, statistics.median(ms_t))
        del x


def bench_loss(launches, warmup, n=55, k=249):
    from video_classification_amd._lib import HipBackend
    from video_classification_amd.input_pipeline import draw_mix
    be = HipBackend()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    z = torch.randn(n, k, generator=g).to(DEV)
    y = torch.randint(0, k, (n,), generator=g).to(DEV)
    rows = draw_mix(n, 192, 192, 0.8, 1.0, generator=g).to(DEV)
    dl, lo, ls = torch.empty(n, k, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    co = torch.zeros(1, dtype=torch.int32, device=DEV)
    variants = {"sfk_softmax_ce": be.softmax_ce(z, y, n, k, 1.0, dl, lo, ls, co),
                "sfk_softmax_ce_mix rows NULL eps 0": be.softmax_ce_mix(z, y, None, 0.0, n, k, 1.0, dl, lo, ls, co),
                "sfk_softmax_ce_mix rows eps 0.1": be.softmax_ce_mix(z, y, rows, 0.1, n, k, 1.0, dl, lo, ls, co)}
    for _ in range(warmup):
        for run in variants.values():
            run(st)
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(launches):
        for name, run in variants.items():
            ms[name].append(_timed(lambda: run(st)))
    base = statistics.median(ms["sfk_softmax_ce"])
    for name in variants:
        emit({"bench": "softmax_ce_mix_kernel", "variant": name, "shape": [n, k], "launches": launches, **_spread(ms[name]),
              "vs_sfk_softmax_ce": round(statistics.median(ms[name]) / base, 3)})


def bench_step(which, reps, rounds):
    from torch.utils.data.dataloader import default_collate
    from video_classification_amd.config import get_cfg
    with tempfile.TemporaryDirectory() as root:
        cfg = get_cfg()
        cfg.CHALEARN.ROOT = root
        cfg.MODEL.DTYPE = "bf16"
        cfg.MODEL.LABEL_SMOOTHING, cfg.MODEL.MIXUP_ALPHA, cfg.MODEL.CUTMIX_ALPHA = 0.1, 0.8, 1.0
        cfg.NUM_CPU = 0
        if which == "htah":
            from video_classification_amd.train import SyntheticChalearn, Trainer
            cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN = 55, 20
            cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT = "slowfast-HTAH", "CropHTAH"
            n = 55
            tr = SyntheticChalearn(cfg, "train", num_videos=n, seed=1, as_uint8=True, frames_per_video=(20, 40))
            te = SyntheticChalearn(cfg, "test", num_videos=1, seed=2, frames_per_video=(20, 20))
            t = Trainer(cfg, train_set=tr, test_set=te, device=DEV)
            clip = [n, 20, 21, 192, 192]
        else:
            from video_classification_amd import gesture_v2 as v2
            cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN, cfg.MODEL.INPUT_SIZE = 10, 20, 192
            n = 10
            tr = v2.SyntheticGesture(cfg, "train", num_videos=n, seed=1)
            te = v2.SyntheticGesture(cfg, "test", num_videos=1, clips_per_video=(1, 1), seed=2)
            t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
            clip = [n, 20, 7, 192, 192]
        t.model.train()
        host = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in default_collate([tr[i] for i in range(n)]).items()}
        eng = t.model.engine
        on = t.step
        eps, t.label_smoothing = t.label_smoothing, 0.0
        off = t._make_step(eng, False, None)                                  # the same engine with every key at its default
        t.label_smoothing = eps
        gen = t._mix_generator()

        def step(keys_on):
            batch, kw = host, {}
            if keys_on:
                batch, kw["mix"] = t._attach_mix(host, gen)
            x, y = t.mm.prepare_data(batch)
            (on if keys_on else off)(x[0], x[1], y, slow_t_index=t.model.slow_t_index, **kw)

        def run(keys_on, k):
            for _ in range(k):
                step(keys_on)
            torch.cuda.synchronize()
        run(False, 2), run(True, 2)
        ms = {False: [], True: []}
        for _ in range(rounds):
            for keys_on in (False, True):
                t0 = time.perf_counter()
                run(keys_on, reps)
                ms[keys_on].append((time.perf_counter() - t0) / reps * 1e3)
        emit({"bench": "mix_step", "geometry": which, "dtype": "bf16", "clip": clip, "reps": reps, "rounds": rounds,
              "keys_off_step": _spread(ms[False]), "keys_on_step": _spread(ms[True]),
              "on_over_off": round(statistics.median(ms[True]) / statistics.median(ms[False]), 4),
              "keys_on": "LABEL_SMOOTHING 0.1, MIXUP_ALPHA 0.8, CUTMIX_ALPHA 1.0 (one draw_mix on the host, the table's H2D, one "
                         "sfk_clip_mix, sfk_softmax_ce_mix for sfk_softmax_ce)"})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "loss", "step_htah", "step_v2"])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the rows to this file as well")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mix.py measures on a GPU; there is no CPU path"
    for w in a.what:
        if w == "kernel":
            bench_kernel(a.launches, a.warmup)
        elif w == "loss":
            bench_loss(a.launches, a.warmup)
        elif w in ("step_htah", "step_v2"):
            bench_step(w[5:], a.reps, a.rounds)
        else:
            raise SystemExit(f"unknown bench {w!r}")
    if a.out:
        with open(a.out, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")
