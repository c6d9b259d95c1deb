"""The grouped optimizer launch (include/sfk_groups.h) on one MI355X at the arena of the benchmark model (SlowFast-R50 8x8, 400
classes, bf16): sfk_adam_hp, sfk_adam_groups with one all-covering group, and sfk_adam_groups with only blocks.4 and the head
covered (Engine.param_segments with blocks.0 .. blocks.3 frozen), next to the covered bytes.  One process; after a warm-up the
variants alternate; every launch is timed on its own with events; median [min, max] over `--launches` launches each.  One JSON
line per variant (kept in profiles/groups_bench.jsonl).
Usage: python tools/bench_groups.py [--launches 60] [--warmup 3] [--parent-lib LIB]
--parent-lib: a shared library with the parent commit's sfk_adam_hp -- that commit's csrc/optim_sched.hip compiled alone
(hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Iinclude -Ivideo-classification_amd/csrc -shared) -- timed first, beside this
build's, in the same process."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s
LOWER = ("blocks.0.", "blocks.1.", "blocks.2.", "blocks.3.")


def launch_part(eng, args):
    be, dev, numel = eng.be, eng.device, eng.arena_numel
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(numel, generator=g, device=dev) * 0.05
    grad = torch.randn(numel, generator=g, device=dev) * 1e-3
    m, v = torch.zeros(numel, device=dev), torch.zeros(numel, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    table = torch.full((1000,), 1e-4, device=dev)
    rows = table.reshape(1, -1).contiguous()
    b1, b2, eps = 0.9, 0.999, 1e-8
    dc = eng.fc_b_off
    all_t = be.group_table([(0, dc, 0, 1), (dc, numel, 0, 0)], [0.05], numel, dev)
    top = eng.param_segments((), LOWER, "weights")
    top_t = be.group_table(top, [0.05], numel, dev)
    covered = sum(e - b for b, e, _, _ in top)
    variants = {
        "sfk_adam_hp": (be.adam_hp(p, grad, m, v, numel, table, b1, b2, eps, 1.0, step, None, weight_decay=0.05,
                                   decay_mode="decoupled", decay_count=dc), numel, 1),
        "sfk_adam_groups all covered": (be.adam_groups(p, grad, m, v, numel, all_t, rows, b1, b2, eps, 1.0, step, None,
                                                       decay_mode="decoupled"), numel, 2),
        "sfk_adam_groups blocks.4 + head": (be.adam_groups(p, grad, m, v, numel, top_t, rows, b1, b2, eps, 1.0, step, None,
                                                           decay_mode="decoupled"), covered, len(top)),
    }
    if args.parent_lib:
        # sfk_adam_hp as the PARENT commit built it (its csrc/optim_sched.hip compiled alone into a side library: FMA
        # contraction as it was), same arguments, through the same binding
        import ctypes as C
        from video_classification_amd import _lib
        plib = C.CDLL(args.parent_lib)
        plib.sfk_adam_hp.argtypes = _lib.SIGNATURES_OPTIM["sfk_adam_hp"]
        hp = be._optim_hp(table, 0.05, "decoupled", dc, None)

        def parent_run(stream, _keep=(hp, plib)):
            rc = plib.sfk_adam_hp(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), numel, C.byref(hp), b1, b2, eps, 1.0,
                                  step.data_ptr(), None, 0, stream)
            assert rc == 0, rc
        variants = dict([("sfk_adam_hp (parent build)", (parent_run, numel, 1))] + list(variants.items()))
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(args.warmup):
        for run, _, _ in variants.values():
            run(st)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.launches):
        for k, (run, _, _) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(st)
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    base = statistics.median(ms["sfk_adam_hp"])
    for k, (_, elems, nsegs) in variants.items():
        med = statistics.median(ms[k])
        nbytes = 7 * 4 * elems
        print(json.dumps({"part": "launch", "variant": k, "numel": numel, "covered": elems, "segments": nsegs,
                          "launches": args.launches, "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4),
                          "ms_max": round(max(ms[k]), 4), "vs_sfk_adam_hp": round(med / base, 4), "bytes": nbytes,
                          "hbm_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="a shared library holding the parent commit's sfk_adam_hp, timed beside this build's")
    args = ap.parse_args()
    from video_classification_amd.slowfast import slowfast_r50_8x8
    model = slowfast_r50_8x8(400, dtype=torch.bfloat16, device="cuda", seed=0)
    launch_part(model.engine, args)


if __name__ == "__main__":
    main()
