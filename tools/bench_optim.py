"""The optimizer launches of include/sfk_optim.h beside sfk_adam, at the arena size of the benchmark model (SlowFast-R50 8x8,
400 classes): sfk_adam, sfk_adam_hp with everything off, with decoupled decay of the weights, with a clipping coefficient, and
sfk_grad_norm alone.  One process; after a warm-up the variants alternate round by round, each round times `--iters`
back-to-back launches with events; per variant the median [min, max] over the rounds, the bytes the launch must move and the
fraction of HBM peak.  Prints one JSON line per variant (kept in profiles/optim_bench.jsonl).
Usage: python tools/bench_optim.py [--rounds 9] [--iters 10] [--warmup 3] [--numel N]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numel", type=int, default=0, help="arena elements; 0 = arena_numel of the benchmark model")
    args = ap.parse_args()
    from video_classification_amd._lib import HipBackend
    dev = "cuda"
    be = HipBackend()
    numel, dc = args.numel, 0
    if numel <= 0:
        from video_classification_amd.slowfast import slowfast_r50_8x8
        eng = slowfast_r50_8x8(400, dtype=torch.bfloat16, device=dev, seed=0).engine
        numel, dc = eng.arena_numel, eng.fc_b_off
        del eng
        torch.cuda.empty_cache()
    dc = dc or numel - numel // 64
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(numel, generator=g, device=dev) * 0.05
    grad = torch.randn(numel, generator=g, device=dev) * 1e-3
    m, v = torch.zeros(numel, device=dev), torch.zeros(numel, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    table = torch.full((1000,), 1e-4, device=dev)
    parts = torch.zeros(be.grad_norm_parts(numel), dtype=torch.float64, device=dev)
    out = torch.ones(2, device=dev)
    b1, b2, eps = 0.9, 0.999, 1e-8
    variants = {
        "sfk_adam": (be.adam(p, grad, m, v, numel, 1e-4, b1, b2, eps, 1.0, step, None), 7),
        "sfk_adam_hp off": (be.adam_hp(p, grad, m, v, numel, table, b1, b2, eps, 1.0, step, None), 7),
        "sfk_adam_hp decoupled decay": (be.adam_hp(p, grad, m, v, numel, table, b1, b2, eps, 1.0, step, None, weight_decay=0.05,
                                                   decay_mode="decoupled", decay_count=dc), 7),
        "sfk_adam_hp clip_coef": (be.adam_hp(p, grad, m, v, numel, table, b1, b2, eps, 1.0, step, None, clip_coef=out[1:2]), 7),
        "sfk_grad_norm": (be.grad_norm(grad, numel, 1.0, 1.0, parts, out), 1),
    }
    st = torch.cuda.current_stream().cuda_stream

    def timed(run):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            run(st)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    for _ in range(args.warmup):
        for run, _passes in variants.values():
            run(st)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (run, _passes) in variants.items():
            ms[k].append(timed(run))
    for k, (run, passes) in variants.items():
        med = statistics.median(ms[k])
        nbytes = passes * numel * 4
        print(json.dumps({"variant": k, "numel": numel, "decay_count": dc if "decay" in k else 0, "rounds": args.rounds,
                          "iters": args.iters, "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4),
                          "ms_max": round(max(ms[k]), 4), "arena_passes": passes, "bytes": nbytes,
                          "hbm_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}))


if __name__ == "__main__":
    main()
