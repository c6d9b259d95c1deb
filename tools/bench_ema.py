"""The weight EMA (include/sfk_ema.h) on one MI355X at the benchmark model (SlowFast-R50 8x8, 400 classes, bf16).
(a) sfk_ema_update and sfk_ema_swap over the model's own arena (34 570 400 elements) and its 220-tensor table of running
    statistics, beside sfk_adam over the same arena in the same process: after a warm-up the variants alternate, every launch
    is timed on its own with events; median [min, max] over `--launches` launches each, the bytes the launch must move (12 per
    element for the average, 28 for Adam) and the fraction of HBM peak.  `--numel N` times a bare arena of N elements with
    no table instead.
(b) the eager bf16 TrainStep at the benchmark geometry (32 clips of 3 x 32 x 224^2) with ema_decay 0 and 0.9999, each in a
    fresh process, `--rounds` times alternating; bench.py's clock (warm-up steps, then `--steps` steps between two
    synchronisations).
One JSON line per variant (kept in profiles/ema_bench.jsonl).
Usage: python tools/bench_ema.py [--launches 60] [--warmup 3] [--numel N] [--rounds 2] [--steps 20] [--part a|b|ab]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s


def launch_part(args):
    from video_classification_amd._lib import HipBackend
    dev = torch.device("cuda", 0)
    be = HipBackend()
    if args.numel > 0:
        numel, table, stat_elems = args.numel, None, 0
        g = torch.Generator(device=dev).manual_seed(0)
        p = torch.randn(numel, generator=g, device=dev) * 0.05
        e = p.clone()
        ema_step = torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        from video_classification_amd.slowfast import slowfast_r50_8x8
        eng = slowfast_r50_8x8(400, dtype=torch.bfloat16, device=dev, seed=0).engine
        eng.optim_state("ema")
        numel, table, p, e, ema_step = eng.arena_numel, eng.ema_table, eng.P.data, eng.ema_P, eng.ema_step
        stat_elems = int(eng.ema_stats.numel())
    g = torch.Generator(device=dev).manual_seed(1)
    grad = torch.randn(numel, generator=g, device=dev) * 1e-3
    m, v = torch.zeros(numel, device=dev), torch.zeros(numel, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ntensors = table.ntensors if table is not None else 0
    variants = {
        "sfk_adam": (be.adam(p, grad, m, v, numel, 1e-4, 0.9, 0.999, 1e-8, 1.0, step, None), 7 * 4 * numel),
        "sfk_ema_update": (be.ema_update(p, e, numel, table, 0.9999, True, ema_step), 3 * 4 * (numel + stat_elems)),
        "sfk_ema_swap": (be.ema_swap(p, e, numel, table), 4 * 4 * (numel + stat_elems)),
    }
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(args.warmup):
        for run, _ in variants.values():
            run(st)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.launches):
        for k, (run, _) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(st)
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    frac = {}
    for k, (_, nbytes) in variants.items():
        med = statistics.median(ms[k])
        frac[k] = nbytes / (med * 1e-3) / HBM_PEAK
        print(json.dumps({"part": "launch", "variant": k, "numel": numel, "table_tensors": ntensors if "ema" in k else 0,
                          "table_elements": stat_elems if "ema" in k else 0, "launches": args.launches,
                          "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                          "bytes": nbytes, "hbm_fraction": round(frac[k], 3),
                          "bandwidth_vs_sfk_adam": round(frac[k] / frac["sfk_adam"], 4)}), flush=True)


def step_child(args):
    """one fresh process: the eager bf16 TrainStep of bench.py with the given ema_decay"""
    from video_classification_amd.slowfast import pack_pathway_index, slowfast_r50_8x8
    from video_classification_amd.train import TrainStep
    dev = torch.device("cuda", 0)
    model = slowfast_r50_8x8(400, dtype=torch.bfloat16, device=dev, seed=0)
    model.train()
    gen = torch.Generator().manual_seed(1234)
    frames = torch.randn(32, 3, 32, 224, 224, generator=gen).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, 400, (32,), generator=gen).to(dev)
    idx = pack_pathway_index(32, 4, dev)
    step = TrainStep(model.engine, lr=2e-4, ema_decay=args.child_decay, ema_warmup=True)
    for _ in range(args.step_warmup):
        step(frames, frames, labels, slow_t_index=idx)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(frames, frames, labels, slow_t_index=idx)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"part": "step", "ema_decay": args.child_decay, "steps": args.steps, "warmup": args.step_warmup,
                      "ms_per_step": round(dt / args.steps * 1e3, 3), "clips_per_sec": round(args.steps * 32 / dt, 2),
                      "loss_after": round(float(step.loss[0]), 4)}), flush=True)


def step_part(args):
    for r in range(args.rounds):
        for decay in (0.0, 0.9999):
            cmd = [sys.executable, os.path.abspath(__file__), "--child-decay", str(decay), "--steps", str(args.steps),
                   "--step-warmup", str(args.step_warmup)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    print(json.dumps(dict(json.loads(line), round=r)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numel", type=int, default=0, help="a bare arena of this many elements, no table; 0 = the benchmark model's")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--child-decay", type=float, default=None, help="(internal) run one step timing in this process")
    args = ap.parse_args()
    if args.child_decay is not None:
        return step_child(args)
    if "b" in args.part:          # first: this process has not opened the GPU yet, the children run alone
        step_part(args)
    if "a" in args.part:
        launch_part(args)


if __name__ == "__main__":
    main()
