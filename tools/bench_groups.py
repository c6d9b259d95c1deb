"""The grouped optimizer launch (include/sfk_groups.h) on one MI355X at the arena of the benchmark model (SlowFast-R50 8x8, 400
classes, bf16): sfk_adam_hp, sfk_adam_groups with one all-covering group, and sfk_adam_groups with only blocks.4 and the head
covered (Engine.param_segments with blocks.0 .. blocks.3 frozen), next to the covered bytes.  One process; after a warm-up the
variants alternate; every launch is timed on its own with events; median [min, max] over `--launches` launches each.  One JSON
line per variant (kept in profiles/groups_bench.jsonl).

`--mode step`: whole eager TrainSteps at the benchmark geometry (32 clips of 32 x 224 x 224, bf16, one process; no step is
captured): the hp step with a constant lr_table and no groups (the same-build baseline), one all-covering group,
freeze=['blocks.0.'] (the stems and fusion 0), freeze=['blocks.0.', 'blocks.1.'], and everything frozen but blocks.4. and the
head.  The variants share one engine and alternate over `--rounds` rounds: each window sets its frozen set (the train plan is
rebuilt into the engine's buffers), warms up, then times `--steps` steps between two device events around synchronised
windows.  One JSON line per variant: ms per step (median [min, max] of the rounds' windows), kernel launches per step by
`kind` counted from the plan's meta, and the covered elements (kept in profiles/groups_step_bench.jsonl).
Usage: python tools/bench_groups.py [--mode launch|step] [--launches 60] [--warmup 3] [--parent-lib LIB] [--rounds 3] [--steps 8]
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


def step_part(model, args):
    from collections import Counter

    from video_classification_amd.slowfast import pack_pathway_index
    from video_classification_amd.train import TrainStep
    eng, dev = model.engine, model.engine.device
    model.train()
    gen = torch.Generator().manual_seed(1234)
    frames = torch.randn(args.batch, 3, 32, 224, 224, generator=gen).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, 400, (args.batch,), generator=gen).to(dev)
    idx = pack_pathway_index(32, 4, dev)
    table = [2e-4] * 1000
    top = [k for k, _, _ in eng.param_tensors() if not k.startswith(("blocks.4.", eng.wiring.head_key))]
    variants = {
        "hp step (lr_table, no groups)": {},
        "one all-covering group": dict(param_groups=[("blocks.", 1.0)]),
        "freeze blocks.0.": dict(freeze=["blocks.0."]),
        "freeze blocks.0. blocks.1.": dict(freeze=["blocks.0.", "blocks.1."]),
        "train blocks.4. + head only": dict(freeze=["blocks.0.", "blocks.1.", "blocks.2.", "blocks.3."]),
    }
    assert eng.frozen_param_keys(variants["train blocks.4. + head only"]["freeze"]) == frozenset(top)
    ms, info = {k: [] for k in variants}, {}
    # one TrainStep per variant, built once, all on ONE trunk stream (TrainStep(trunk=)): with a new high-priority stream per
    # window some windows of EVERY variant, the baseline included, ran about 10 ms a step slower than the others (27.6 against
    # 38 .. 41.5 ms for the hp step: profiles/groups_step_bench.jsonl, part "step-new-stream-per-window")
    steps = {}
    for name, kw in variants.items():
        steps[name] = TrainStep(eng, lr=2e-4, lr_table=table, trunk=next(iter(steps.values())).trunk if steps else None, **kw)
    for _ in range(args.rounds):
        for name, kw in variants.items():
            step = steps[name]                                          # its first call puts its frozen set back: the warm-up rebuilds the plan
            for _ in range(args.warmup):
                step(frames, frames, labels, slow_t_index=idx)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step(frames, frames, labels, slow_t_index=idx)
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / args.steps)
            if name not in info:
                pl = eng._plan_for(frames, frames, idx, True)
                ops = next(iter(step._cache.values()))["ops"]
                kinds = Counter(m["kind"] for ol in (pl.fwd, pl.bwd) for m in ol.meta if m is not None)
                info[name] = dict(launches_by_kind=dict(sorted(kinds.items())), described_launches=sum(kinds.values()),
                                  fwd_ops=len(pl.fwd), bwd_ops=len(pl.bwd), step_ops=sorted(ops),
                                  covered=sum(e - b_ for b_, e, _, _ in step.opt.segments) if step.opt.grouped else eng.arena_numel,
                                  segments=len(step.opt.segments) if step.opt.grouped else 1, loss=round(float(step.loss[0]), 4))
    base, allc = statistics.median(ms["hp step (lr_table, no groups)"]), statistics.median(ms["one all-covering group"])
    for name in variants:
        med = statistics.median(ms[name])
        print(json.dumps(dict({"part": "step", "variant": name, "batch": args.batch, "numel": eng.arena_numel, "rounds": args.rounds,
                               "steps_per_window": args.steps, "ms_per_step_median": round(med, 3),
                               "ms_per_step_min": round(min(ms[name]), 3), "ms_per_step_max": round(max(ms[name]), 3),
                               "ms_per_step_windows": [round(x, 3) for x in ms[name]],
                               "vs_hp_step": round(med / base, 4), "vs_all_covering": round(med / allc, 4)}, **info[name])),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("launch", "step"), default="launch")
    ap.add_argument("--rounds", type=int, default=3, help="step mode: windows per variant")
    ap.add_argument("--steps", type=int, default=8, help="step mode: timed steps per window")
    ap.add_argument("--batch", type=int, default=32, help="step mode: clips")
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="a shared library holding the parent commit's sfk_adam_hp, timed beside this build's")
    args = ap.parse_args()
    from video_classification_amd.slowfast import slowfast_r50_8x8
    model = slowfast_r50_8x8(400, dtype=torch.bfloat16, device="cuda", seed=0)
    if args.mode == "step":
        return step_part(model, args)
    launch_part(model.engine, args)


if __name__ == "__main__":
    main()
