"""The grouped TrainStep (param_groups= / freeze=) against the contract of include/sfk_groups.h, inside ONE
run: before every step P and the optimizer state are snapshotted, after it G is read, and for every segment of the step's
table a reference backend's adam_hp / sgd_hp runs on clones of the slices with the group's rate row, the group's decay and a
counter holding step - 1.  P and the state must hold those bits, elements in no segment their earlier bits, the device counter
the step number; with clipping the norm and the coefficient are the reference's grad_norm of G with the uncovered elements
zeroed.  Only quantities of the same run are compared (filter gradients use atomics on the GPU), so the same function serves
the emulated backend (tests/test_groups_step_cpu.py) and HipBackend (tests/test_gpu_groups_step.py).  Also: what the pruned
train plans are checked for on both."""
import torch

import head_ref64 as H

GROUPS = [("blocks.1.", 0.1), ("@fresh", 0.5, 0.0)]
FREEZE = ["blocks.0."]
TABLE = [1e-3, 3e-3, 2e-3, 5e-4]


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32).cpu()


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(bits(a), bits(b))


def mark_fresh(eng):
    """as after a pretrained load that left the head and res5's BatchNorms untouched: '@fresh' / '@pretrained' both match"""
    eng.fresh_keys = [k for k, _, _ in eng.param_tensors()
                      if k.startswith(eng.wiring.head_key) or (k.startswith("blocks.4.") and ".norm" in k)]


def covered_mask(segments, count, device) -> torch.Tensor:
    keep = torch.zeros(count, dtype=torch.bool, device=device)
    for b, e, _, _ in segments:
        keep[b:e] = True
    return keep


def _sync(eng):
    if eng.device.type == "cuda":
        torch.cuda.synchronize()


def _state(eng, sgd):
    names = ("sgd_buf",) if sgd else ("adam_m", "adam_v")
    return [torch.zeros_like(eng.P.data) if getattr(eng, n) is None else getattr(eng, n).clone() for n in names]


def check_grouped_steps(step, run_step, ref_be, steps: int):
    """run_step() `steps` times on `step` (a grouped TrainStep); the verdicts described above, H.Exact each"""
    eng, opt = step.eng, step.opt
    sgd = opt.optimizer == "sgd"
    assert opt.grouped and opt.segments
    n, dev, st = eng.arena_numel, eng.device, eng._stream()
    keep = covered_mask(opt.segments, n, dev)
    rows, wds = opt.lr_rows, opt.group_decays
    vs = [H.Exact("row 0 is the hp route's table", same(rows[0], opt.lr_table)),
          H.Exact("something is frozen and something is not", 0 < int(keep.sum()) < n)]
    for s in range(1, steps + 1):
        P0, S0 = eng.P.data.clone(), _state(eng, sgd)
        run_step()
        _sync(eng)
        G = eng.G.clone()
        P1, S1 = eng.P.data.clone(), _state(eng, sgd)
        coef = None
        if opt.clip_grad_norm > 0:
            out = torch.zeros(2, device=dev)
            parts = torch.zeros(ref_be.grad_norm_parts(n), dtype=torch.float64, device=dev)
            ref_be.grad_norm(torch.where(keep, G, torch.zeros_like(G)), n, 1.0, opt.clip_grad_norm, parts, out)(st)
            _sync(eng)
            vs.append(H.Exact(f"step {s} norm and coefficient", same(out, eng.grad_norm), f"{out.tolist()} {eng.grad_norm.tolist()}"))
            coef = out[1:2]
        ok_p = ok_s = True
        for b, e, grp, dec in opt.segments:
            p, g = P0[b:e].clone(), G[b:e].clone()
            state = [t[b:e].clone() for t in S0]
            ctr = torch.full((1,), s - 1, dtype=torch.int64, device=dev)
            kw = dict(weight_decay=wds[grp], decay_mode=opt.decay_mode, decay_count=e - b if dec else 0, clip_coef=coef)
            if sgd:
                ref_be.sgd_hp(p, g, state[0], e - b, rows[grp], opt.momentum, opt.dampening, opt.nesterov, 1.0, ctr, None, **kw)(st)
            else:
                ref_be.adam_hp(p, g, state[0], state[1], e - b, rows[grp], opt.betas[0], opt.betas[1], opt.eps, 1.0, ctr, None,
                               **kw)(st)
            _sync(eng)
            ok_p = ok_p and same(p, P1[b:e])
            ok_s = ok_s and all(same(a, t[b:e]) for a, t in zip(state, S1))
        vs.append(H.Exact(f"step {s} P on every segment", ok_p))
        vs.append(H.Exact(f"step {s} state on every segment", ok_s))
        vs.append(H.Exact(f"step {s} frozen P keeps its bits", same(P0[~keep], P1[~keep])))
        vs.append(H.Exact(f"step {s} frozen state keeps its bits", all(same(a[~keep], b_[~keep]) for a, b_ in zip(S0, S1))))
        vs.append(H.Exact(f"step {s} covered P moved", not same(P0[keep], P1[keep])))
        vs.append(H.Exact(f"step {s} counter", int(opt._counter()[0]) == s))
    return vs


def rejected(vs) -> bool:
    return any(not v.ok for v in vs)


def report(vs):
    for v in vs:
        print(v)
    bad = [v for v in vs if not v.ok]
    assert not bad, bad


# ------------------------------------------------------------------ pruned plans
def train_plan(eng):
    plans = [pl for key, pl in eng._plans.items() if key[3]]
    assert len(plans) == 1
    return plans[0]


def bwd_kinds(pl):
    """(kind, layer) of every backward op that carries a description, in issue order"""
    return [(m["kind"], m.get("layer")) for m in pl.bwd.meta if m is not None]


def joins(pl):
    from video_classification_amd.engine import Wait
    return [(op.lane, op.on) for op in pl.bwd if isinstance(op, Wait)]


def marked_mask(pl, count, device) -> torch.Tensor:
    """the arena elements some emitted writer finishes (Plan.grad_marks); the ranges must be disjoint"""
    hit = torch.zeros(count, dtype=torch.int32, device=device)
    for _, (off, n) in pl.grad_marks:
        hit[off:off + n] += 1
    assert int(hit.max()) <= 1
    return hit > 0


def under(layer, prefixes) -> bool:
    return layer is not None and any(str(layer).startswith(p) for p in prefixes)
