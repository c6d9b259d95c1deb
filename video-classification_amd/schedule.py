"""Learning-rate schedules as per-step tables (pure host code).

``TrainStep(lr_table=...)`` sends the table to the device once; optimizer step s (1-based, the counter the optimizer launch
keeps on the device) reads entry min(s, len) - 1 (include/sfk_optim.h), so entry k is the rate of the (k+1)-th
``optimizer.step()`` of a torch loop that calls ``scheduler.step()`` after it.  The index is the optimizer's step count since
its construction: as in the reference, neither the optimizer state nor the schedule position is checkpointed, so a resumed
run starts the table again.  Past the table's end the last rate holds.

Each function states torch's scheduler in closed form, evaluated in double per step:
  constant   the flat table;
  cosine     SequentialLR([LinearLR(start_factor=1/warmup, end_factor=1, total_iters=warmup),
                           CosineAnnealingLR(T_max=total - warmup, eta_min=lr_min)], milestones=[warmup]);
             warmup = 0: CosineAnnealingLR(T_max=total, eta_min=lr_min) alone;
  multistep  MultiStepLR(milestones (epochs), gamma) stepped once per epoch, each epoch's rate repeated steps_per_epoch times.
"""
from __future__ import annotations

import bisect
import math
from typing import List, Sequence

SCHEDULES = ("constant", "cosine", "multistep")


def constant_table(lr: float, total_steps: int) -> List[float]:
    return [float(lr)] * max(int(total_steps), 1)


def cosine_table(lr: float, total_steps: int, warmup_steps: int = 0, lr_min: float = 0.0) -> List[float]:
    total, w = max(int(total_steps), 1), int(warmup_steps)
    if w < 0 or w >= total and w > 0:
        raise ValueError(f"warmup_steps={warmup_steps}: 0 <= warmup < total steps ({total})")
    t_max = total - w
    out = []
    for k in range(total):
        if k < w:
            out.append(lr * (1.0 / w + (1.0 - 1.0 / w) * k / w))
        else:
            out.append(lr_min + (lr - lr_min) * (1.0 + math.cos(math.pi * (k - w) / t_max)) / 2.0)
    return out


def multistep_table(lr: float, epochs: int, steps_per_epoch: int, milestones: Sequence[int], gamma: float = 0.1) -> List[float]:
    ms = sorted(int(m) for m in milestones)
    spe = max(int(steps_per_epoch), 1)
    out = []
    for e in range(max(int(epochs), 1)):
        out.extend([lr * gamma ** bisect.bisect_right(ms, e)] * spe)
    return out


def lr_schedule(name: str, lr: float, epochs: int, steps_per_epoch: int, warmup_steps: int = 0, lr_min: float = 0.0,
                milestones: Sequence[int] = (), gamma: float = 0.1) -> List[float]:
    """the table of `epochs * steps_per_epoch` rates of schedule `name` ('constant' | 'cosine' | 'multistep')"""
    name = str(name).lower()
    total = max(int(epochs), 1) * max(int(steps_per_epoch), 1)
    if name == "constant":
        return constant_table(lr, total)
    if name == "cosine":
        return cosine_table(lr, total, warmup_steps, lr_min)
    if name == "multistep":
        return multistep_table(lr, epochs, steps_per_epoch, milestones, gamma)
    raise ValueError(f"LR_SCHEDULE={name!r}: one of {SCHEDULES}")


def optim_kwargs(cfg, steps_per_epoch) -> dict:
    """MODEL.LR_SCHEDULE / LR_* / WEIGHT_DECAY* / CLIP_GRAD_NORM as TrainStep's keyword arguments; every key at its default gives
    {} (the step then issues the launches it always issued).  steps_per_epoch: an int, or a callable asked only when a
    schedule needs it (a train loader without a length serves every constant-rate run)."""
    m = cfg.MODEL
    kw = {}
    name = str(m.get("LR_SCHEDULE", "constant")).lower()
    if name not in SCHEDULES:
        raise ValueError(f"MODEL.LR_SCHEDULE={name!r}: one of {SCHEDULES}")
    warmup = int(m.get("LR_WARMUP_STEPS", 0))
    if name != "constant":
        spe = int(steps_per_epoch() if callable(steps_per_epoch) else steps_per_epoch)
        kw["lr_table"] = lr_schedule(name, float(m.LR), int(m.MAX_EPOCH), spe, warmup, float(m.get("LR_MIN", 0.0)),
                                     list(m.get("LR_MILESTONES", [])), float(m.get("LR_GAMMA", 0.1)))
    wd = float(m.get("WEIGHT_DECAY", 0.0))
    mode = str(m.get("WEIGHT_DECAY_MODE", "decoupled")).lower()
    scope = str(m.get("WEIGHT_DECAY_SCOPE", "weights")).lower()
    if mode not in ("decoupled", "l2"):
        raise ValueError(f"MODEL.WEIGHT_DECAY_MODE={mode!r}: 'decoupled' or 'l2'")
    if scope not in ("weights", "all"):
        raise ValueError(f"MODEL.WEIGHT_DECAY_SCOPE={scope!r}: 'weights' or 'all'")
    if wd < 0:
        raise ValueError(f"MODEL.WEIGHT_DECAY={wd}: must not be negative")
    if wd > 0:
        kw.update(weight_decay=wd, decay_mode=mode, decay_scope=scope)
    clip = float(m.get("CLIP_GRAD_NORM", 0.0))
    if clip < 0:
        raise ValueError(f"MODEL.CLIP_GRAD_NORM={clip}: must not be negative (0 = off)")
    if clip > 0:
        kw["clip_grad_norm"] = clip
    return kw


def group_kwargs(cfg) -> dict:
    """MODEL.PARAM_GROUPS ([selector, lr_mult] or [selector, lr_mult, wd_mult] entries) and MODEL.FREEZE (selectors) as
    TrainStep's `param_groups` / `freeze` keywords; both empty gives {}.  Only the entries' shape is checked here: the
    selectors resolve against the engine (Engine._matcher), the multipliers' range is optim.Optimizer's to refuse."""
    m = cfg.MODEL
    groups, freeze = m.get("PARAM_GROUPS", []), m.get("FREEZE", [])
    if isinstance(groups, str) or not isinstance(groups, (list, tuple)):
        raise ValueError(f"MODEL.PARAM_GROUPS={groups!r}: a list of [selector, lr_mult] or [selector, lr_mult, wd_mult]")
    if isinstance(freeze, str) or not isinstance(freeze, (list, tuple)):
        raise ValueError(f"MODEL.FREEZE={freeze!r}: a list of selectors")
    out = []
    for g in groups:
        ok = isinstance(g, (list, tuple)) and len(g) in (2, 3) and isinstance(g[0], str)
        ok = ok and all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in g[1:])
        if not ok:
            raise ValueError(f"MODEL.PARAM_GROUPS entry {g!r}: [selector, lr_mult] or [selector, lr_mult, wd_mult]")
        out.append((g[0],) + tuple(float(x) for x in g[1:]))
    for s in freeze:
        if not isinstance(s, str):
            raise ValueError(f"MODEL.FREEZE entry {s!r}: a selector (a state_dict() key prefix, '@fresh' or '@pretrained')")
    kw = {}
    if out:
        kw["param_groups"] = out
    if freeze:
        kw["freeze"] = [str(s) for s in freeze]
    return kw
