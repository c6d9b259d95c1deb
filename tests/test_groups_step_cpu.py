"""Parameter groups and frozen layers from the train step up, on the emulated engine: the grouped
optimizer launch of optim.Optimizer against the contract of include/sfk_groups.h inside one run (tests/groups_step_ref.py), the
split pair against the single launch, the train plans Engine.set_frozen prunes, three steps against the oracle with torch's
own param groups, the defaults against today's launches, the config keys, one epoch of each trainer and two ranks over gloo.
tests/test_gpu_groups_step.py runs the same checks on an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import groups_step_ref as S
from emu_groups import EmuGroupsBackend
from emu_optim import EmuOptimBackend
from helpers import rel_err
from optim_trace import LaunchTrace, state_present
from test_dist_cpu import _free_port
from test_engine_cpu import make_inputs, make_models, oracle_train_step_with_engine_mask
from test_groups_cpu import _batch, _mini, _res2d
from video_classification_amd import gesture_v2 as v2
from video_classification_amd import train as v1
from video_classification_amd.optim import Optimizer
from video_classification_amd.train import TrainStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_A = "blocks.2.multipathway_blocks.0.res_blocks.0.branch2.conv_a"
ROUTES = {
    "adam-decoupled": dict(weight_decay=0.1, decay_mode="decoupled"),
    "adam-clip": dict(weight_decay=0.1, decay_mode="decoupled", clip_grad_norm=1.0),
    "sgd-l2": dict(optimizer="sgd", momentum=0.9, weight_decay=0.1, decay_mode="l2"),
}


class IgnoresLrMult(EmuGroupsBackend):
    """mutant: every group reads group 0's rates"""

    def adam_groups(self, p, g, m, v, count, table, lr_rows, *a, **kw):
        return super().adam_groups(p, g, m, v, count, table, lr_rows[:1].expand(lr_rows.shape[0], -1).contiguous(), *a, **kw)


class UpdatesFrozen(EmuGroupsBackend):
    """mutant: the elements no segment covers are updated too"""
    visit_frozen = True


def _grouped(be, steps, freeze=S.FREEZE, **kw):
    m = _mini(backend=be)
    S.mark_fresh(m.engine)
    m.train()
    step = TrainStep(m.engine, lr=1e-3, lr_table=S.TABLE, param_groups=S.GROUPS, freeze=freeze, **kw)
    x, y = _batch()
    vs = S.check_grouped_steps(step, lambda: step(x[:, :5], x[:, 5:], y), EmuOptimBackend(), steps)
    return step, vs


# ------------------------------------------------------------------ 1. bit identity within one run
@pytest.mark.parametrize("route", list(ROUTES))
def test_grouped_step_is_adam_hp_on_every_segment(route):
    step, vs = _grouped(EmuGroupsBackend(), 4, **ROUTES[route])
    ops = next(iter(step._cache.values()))["ops"]
    assert ("grad_norm" in ops) == (route == "adam-clip") and "adam" in ops and "adam_main" not in ops
    groups = {grp for _, _, grp, _ in step.opt.segments}
    assert groups == {0, 1, 2}, groups                                      # the rest, blocks.1., '@fresh'
    assert step.last_lr() == step.last_lrs()[0] and len(step.last_lrs()) == 3
    want = [float(np.float32(S.TABLE[3] * mult)) for mult in (1.0, 0.1, 0.5)]
    assert step.last_lrs() == want, (step.last_lrs(), want)
    S.report(vs)


@pytest.mark.parametrize("backend", [EmuGroupsBackend, IgnoresLrMult, UpdatesFrozen])
def test_the_checks_catch_a_wrong_grouped_launch(backend):
    """one step with, beside the stems, a frozen BatchNorm inside a live block: its gradient is still written (a by-product of
    the block's backward), so a launch that visits frozen ranges moves it -- the pruned stems' gradient is zero and hides that"""
    freeze = S.FREEZE + ["blocks.3.multipathway_blocks.0.res_blocks.0.branch2.norm_c."]
    step, vs = _grouped(backend(), 1, freeze=freeze, **ROUTES["adam-decoupled"])
    keep = S.covered_mask(step.opt.segments, step.eng.arena_numel, step.eng.device)
    assert bool(step.eng.G[~keep].any()), "a frozen range with a gradient"
    bad = {v.name.split(" ", 2)[2] for v in vs if not v.ok}
    want = {EmuGroupsBackend: set(), IgnoresLrMult: {"P on every segment"},
            UpdatesFrozen: {"frozen P keeps its bits", "frozen state keeps its bits"}}[backend]
    assert bad == want and S.rejected(vs) == bool(want), vs


# ------------------------------------------------------------------ 2. the split pair
def _grouped_opt(eng):
    S.mark_fresh(eng)
    return Optimizer(eng, lr=1e-3, lr_table=S.TABLE, weight_decay=0.1, decay_mode="decoupled", param_groups=S.GROUPS,
                     freeze=S.FREEZE)


@pytest.mark.parametrize("where", ["inside a segment", "inside a frozen gap"])
def test_split_pair_equals_the_single_launch(where):
    one, two = _mini(backend=EmuGroupsBackend()).engine, _mini(backend=EmuGroupsBackend()).engine
    o1, o2 = _grouped_opt(one), _grouped_opt(two)
    assert o2.can_split
    b, e = o2.segments[0][:2]
    assert b > 0, "the frozen stems' filters open the arena"
    cut = (b + e) // 2 // 4 * 4 + 1 if where == "inside a segment" else one.layers[1].w_off
    assert (b < cut < e) if where == "inside a segment" else (0 < cut < b)
    single = o1.update_ops()
    main, tail, set_tail = o2.split_ops(cut)
    assert sorted(o2._tables) == [(0, cut), (cut, two.arena_numel)]
    covered = sum(e_ - b_ for t in o2._tables.values() for b_, e_, _, _ in t.segments)
    assert covered == sum(e_ - b_ for b_, e_, _, _ in o1.segments)
    gen = torch.Generator().manual_seed(3)
    P0 = one.P.data.clone()
    for s in (1, 2):
        g = torch.randn(one.arena_numel, generator=gen)
        one.G.copy_(g)
        two.G.copy_(g)
        single(0)
        main(0)
        set_tail()
        assert int(two.adam_step[0]) == s and int(two.adam_step_tail[0]) == s - 1
        tail(0)
        assert int(one.adam_step[0]) == int(two.adam_step[0]) == int(two.adam_step_tail[0]) == s
        for a, b_ in ((one.P.data, two.P.data), (one.adam_m, two.adam_m), (one.adam_v, two.adam_v)):
            assert S.same(a, b_), (where, s)
    keep = S.covered_mask(o1.segments, one.arena_numel, one.device)
    assert S.same(one.P.data[~keep], P0[~keep]) and not S.same(one.P.data[keep], P0[keep])
    assert not bool(one.adam_m[~keep].any()) and not bool(one.adam_v[~keep].any())


# ------------------------------------------------------------------ 3. the pruned plan
PRUNED = {
    "stems": ["blocks.0."],
    "through-res3": ["blocks.0.", "blocks.1.", "blocks.2."],
    "one-filter": [CONV_A + ".weight"],
}
# depth 26 has two blocks per stage: the cut falls INSIDE a stage (_stage_bwd's `take`), on the slow and on the fast pathway
SLOW_B0, FAST_B0 = "blocks.3.multipathway_blocks.0.res_blocks.0.", "blocks.3.multipathway_blocks.1.res_blocks.0."
PRUNED26 = {
    "cut-in-slow-res4": ["blocks.0.", "blocks.1.", "blocks.2.", "blocks.3.multipathway_blocks.1.", "blocks.3.multipathway_fusion",
                         SLOW_B0],
    "cut-in-fast-res4": ["blocks.0.", "blocks.1.", "blocks.2.", "blocks.3.multipathway_fusion", FAST_B0],
}


def _mini26():
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=26, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=torch.float32, device="cpu", backend=EmuGroupsBackend(), seed=0)


def _one_step(freeze, make=None):
    m = (make or (lambda: _mini(backend=EmuGroupsBackend())))()
    m.train()
    for L in m.engine.layers:                            # the block-final gammas start at 0, which zeroes every gradient inside
        if L.cb.zero_init_gamma:                         # the blocks' branches: give the dropped writers something to write
            m.engine.P.data[L.g_off:L.g_off + L.c] = 0.5
    x, y = _batch()
    step = TrainStep(m.engine, lr=1e-3, freeze=freeze) if freeze else TrainStep(m.engine, lr=1e-3)
    step(x[:, :5], x[:, 5:], y)
    return m, step, S.train_plan(m.engine)


@pytest.fixture(scope="module")
def unpruned():
    m, _, pl = _one_step(())
    return dict(G=m.engine.G.clone(), kinds=S.bwd_kinds(pl), joins=S.joins(pl), marks=sorted(r for _, r in pl.grad_marks),
                tail_cut=pl.tail_cut, nbwd=len(pl.bwd))


@pytest.mark.parametrize("case", list(PRUNED))
def test_frozen_set_prunes_the_train_plan(unpruned, case):
    freeze = PRUNED[case]
    m, step, pl = _one_step(freeze)
    eng = m.engine
    kinds = S.bwd_kinds(pl)
    assert unpruned["tail_cut"] is not None and len(unpruned["marks"]) == len(set(unpruned["marks"]))
    if case == "one-filter":
        # (iii) exactly its stand-alone filter gradient goes (with the Wait that handed it its lane); everything else stays
        assert kinds == [k for k in unpruned["kinds"] if k != ("conv_wgrad", CONV_A)]
        assert len(kinds) == len(unpruned["kinds"]) - 1 and len(pl.bwd) == unpruned["nbwd"] - 2
        assert pl.tail_cut is not None and pl.tail_cut[1] == unpruned["tail_cut"][1]
    else:
        # (i), (ii) no stem filter gradient, no split, no backward op of a layer under the frozen prefixes; the joins stay
        assert not [k for k in kinds if k[0] == "stem_wgrad"] and pl.tail_cut is None
        assert not [k for k in kinds if S.under(k[1], freeze)], [k for k in kinds if S.under(k[1], freeze)][:4]
        assert [k for k in unpruned["kinds"] if S.under(k[1], freeze)]
        it = iter(unpruned["kinds"])
        assert all(k in it for k in kinds), "what is left keeps its order"
        assert len(kinds) < len(unpruned["kinds"])
    assert S.joins(pl)[-3:] == unpruned["joins"][-3:] == [(0, 1), (0, 2), (0, 3)]
    # (v) the marks are the unpruned plan's ranges that hold a trainable element, each behind an emitted op
    frozen = eng.frozen_keys
    assert frozen == eng.frozen_param_keys(freeze) and frozen
    live = [(o, o + n) for k, o, n in eng.param_tensors() if k not in frozen]
    want = [(o, n) for o, n in unpruned["marks"] if any(b < o + n and e > o for b, e in live)]
    assert sorted(r for _, r in pl.grad_marks) == want
    from video_classification_amd.engine import Wait
    assert all(0 < i <= len(pl.bwd) and not isinstance(pl.bwd[i - 1], Wait) for i, _ in pl.grad_marks)
    for nseg in (1, 3, 6):
        segs = pl.grad_segments(nseg)
        assert segs[0][0] == 0 and segs[-1][1] == len(pl.bwd) and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert sorted(r for _, _, rs in segs for r in rs) == want
        assert all(i <= end for (_, end, rs) in segs for r in rs for i, rr in pl.grad_marks if rr == r)
    # (iv) same seed, same batch: G equals the unpruned engine's where a writer is left, and is zero where it was dropped
    marked = S.marked_mask(pl, eng.arena_numel, eng.device)
    assert S.same(eng.G[marked], unpruned["G"][marked]) and bool(eng.G[marked].any())
    assert not bool(eng.G[~marked].any()) and bool(unpruned["G"][~marked].any())
    keep = S.covered_mask(step.opt.segments, eng.arena_numel, eng.device)
    assert not bool((keep & ~marked).any()), "every trainable element has a writer"


def test_eval_plans_do_not_depend_on_the_frozen_set():
    m = _mini(backend=EmuGroupsBackend())
    eng = m.engine
    x, _ = _batch()
    m.eval()
    ev = eng.forward(x[:, :5], x[:, 5:], False)
    m.train()
    tr = eng.forward(x[:, :5], x[:, 5:], True)
    eng.set_frozen(["blocks.0.", "blocks.1."])
    assert list(eng._plans.values()) == [ev], "the train plan is dropped, the eval plan stays"
    assert eng.forward(x[:, :5], x[:, 5:], False) is ev
    fresh = _mini(backend=EmuGroupsBackend()).engine
    fresh.set_frozen(["blocks.0.", "blocks.1."])
    ev2 = fresh.forward(x[:, :5], x[:, 5:], False)
    assert ev2.fwd.meta == ev.fwd.meta and ev2.fwd.lane == ev.fwd.lane and len(ev2.bwd) == len(ev.bwd) == 0
    tr2 = eng.forward(x[:, :5], x[:, 5:], True)
    assert tr2 is not tr and tr2.fwd.meta == tr.fwd.meta and len(tr2.bwd) < len(tr.bwd)      # the forward is not pruned
    eng.set_frozen(())
    assert S.bwd_kinds(eng.forward(x[:, :5], x[:, 5:], True)) == S.bwd_kinds(tr)


def test_a_later_step_with_another_frozen_set_resets_the_plans():
    m = _mini(backend=EmuGroupsBackend())
    eng = m.engine
    m.train()
    x, y = _batch()
    a = TrainStep(eng, lr=1e-3, freeze=["blocks.0."])
    a(x[:, :5], x[:, 5:], y)
    first = S.train_plan(eng)
    TrainStep(eng, lr=1e-3, freeze=["blocks.0."])
    assert S.train_plan(eng) is first, "the same set keeps the plans"
    b = TrainStep(eng, lr=1e-3)
    assert eng.frozen_keys == frozenset() and not [k for k in eng._plans if k[3]]
    b(x[:, :5], x[:, 5:], y)
    assert [k for k in S.bwd_kinds(S.train_plan(eng)) if k[0] == "stem_wgrad"]
    # the first step, called again, puts its own set back: it never runs on plans pruned for another set
    a(x[:, :5], x[:, 5:], y)
    assert eng.frozen_keys == eng.frozen_param_keys(["blocks.0."])
    assert not [k for k in S.bwd_kinds(S.train_plan(eng)) if k[0] == "stem_wgrad"]


@pytest.fixture(scope="module")
def unpruned26():
    m, _, pl = _one_step((), _mini26)
    return dict(G=m.engine.G.clone(), kinds=S.bwd_kinds(pl), marks=sorted(r for _, r in pl.grad_marks))


@pytest.mark.parametrize("case", list(PRUNED26))
def test_the_cut_falls_inside_a_stage_at_two_blocks_per_stage(unpruned26, case):
    """(iv), (v) where the last trainable unit is the SECOND block of a stage: its first block, emitted after it, is not"""
    freeze = PRUNED26[case]
    m, step, pl = _one_step(freeze, _mini26)
    eng = m.engine
    kinds = S.bwd_kinds(pl)
    dropped_block = SLOW_B0 if case == "cut-in-slow-res4" else FAST_B0
    kept_block = dropped_block.replace("res_blocks.0.", "res_blocks.1.")
    assert [k for k in unpruned26["kinds"] if S.under(k[1], [dropped_block])] and not [k for k in kinds if S.under(k[1], [dropped_block])]
    assert [k for k in kinds if S.under(k[1], [kept_block])] == [k for k in unpruned26["kinds"] if S.under(k[1], [kept_block])]
    assert not [k for k in kinds if S.under(k[1], ["blocks.0.", "blocks.1.", "blocks.2."])]
    it = iter(unpruned26["kinds"])
    assert all(k in it for k in kinds) and len(kinds) < len(unpruned26["kinds"])
    assert S.joins(pl)[-3:] == [(0, 1), (0, 2), (0, 3)]
    live = [(o, o + n) for k, o, n in eng.param_tensors() if k not in eng.frozen_keys]
    want = [(o, n) for o, n in unpruned26["marks"] if any(b < o + n and e > o for b, e in live)]
    assert sorted(r for _, r in pl.grad_marks) == want
    for nseg in (1, 3, 6):
        segs = pl.grad_segments(nseg)
        assert segs[0][0] == 0 and segs[-1][1] == len(pl.bwd) and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert sorted(r for _, _, rs in segs for r in rs) == want
    marked = S.marked_mask(pl, eng.arena_numel, eng.device)
    assert S.same(eng.G[marked], unpruned26["G"][marked]) and bool(eng.G[marked].any())
    keep = S.covered_mask(step.opt.segments, eng.arena_numel, eng.device)
    assert not bool((keep & ~marked).any()) and bool(unpruned26["G"][~keep].any())
    assert not bool(eng.G[keep & ~marked].any())


# ------------------------------------------------------------------ 4. against the oracle
def _oracle_groups(om, eng, groups, freeze, lr, wd):
    """torch.optim.Adam's param groups from the same selectors: the first matching selector wins, freeze beats groups, the
    decay rule of scope 'weights' (conv filters and the FC weight: every parameter with more than one dimension)"""
    keys = eng._state_keys()
    gm = [(eng._matcher(s, keys), mult) for s, mult in groups]
    fm = [eng._matcher(s, keys) for s in freeze]
    out, rate = {}, {}
    for k, p in om.named_parameters():
        if any(f(k) for f in fm):
            p.requires_grad_(False)
            rate[k] = None
            continue
        mult = next((mu for f, mu in gm if f(k)), 1.0)
        rate[k] = lr * mult
        out.setdefault((mult, p.dim() > 1), []).append(p)
    return [dict(params=ps, lr=lr * mult, weight_decay=wd if dec else 0.0) for (mult, dec), ps in out.items()], rate


def test_three_grouped_steps_match_the_oracle():
    """run_k_steps / assert_k_step_parity of tests/test_engine_cpu.py with groups: the same loop, the same constants, the
    tensor's own group rate in the max-move bound, and frozen tensors equal to their initial values on both sides."""
    lr, wd, k = 2e-4, 1e-2, 3
    groups, freeze = [("blocks.1.", 0.1), ("@fresh", 0.5)], ["blocks.0."]
    om, m = make_models(True, backend=EmuGroupsBackend())
    eng = m.engine
    S.mark_fresh(eng)
    x, labels = make_inputs(True), torch.tensor([1, 4])
    pg, rate = _oracle_groups(om, eng, groups, freeze, lr, wd)
    assert len(pg) >= 5 and sorted({g["lr"] for g in pg}) == sorted({lr * 0.1, lr * 0.5, lr})
    opt = torch.optim.Adam(pg, lr=lr)
    step = TrainStep(eng, lr=lr, weight_decay=wd, decay_mode="l2", decay_scope="weights", param_groups=groups, freeze=freeze)
    before = {kk: v.clone() for kk, v in om.state_dict().items()}
    m.train()
    losses = []
    for _ in range(k):
        _, loss_o = oracle_train_step_with_engine_mask(om, eng, x, labels)
        opt.step()
        losses.append((float(loss_o), float(step(x[0], x[1], labels))))
    assert int(eng.adam_step[0]) == k
    sd_o, sd_m = om.state_dict(), m.state_dict()
    assert set(sd_o) == set(sd_m)
    upd, nfrozen = {}, 0
    for kk in sd_o:
        a, b = sd_o[kk], sd_m[kk]
        if ".residual." in kk or ".res_unit." in kk:
            assert torch.equal(a, b), kk
        elif kk.endswith("num_batches_tracked"):
            assert int(a) == int(b) == k, kk             # frozen BatchNorm layers keep counting: the forward is not pruned
        elif kk.endswith(("running_mean", "running_var")):
            assert rel_err(b, a) < 2e-2, kk
            assert not torch.equal(b, before[kk]), kk    # ... and keep updating their running statistics
        elif rate[kk] is None:
            assert kk.startswith("blocks.0.") and torch.equal(a, before[kk]) and torch.equal(b, before[kk]), kk
            nfrozen += 1
        else:
            uo, um = (a - before[kk]).flatten().double(), (b - before[kk]).flatten().double()
            cos = float(uo @ um / (uo.norm() * um.norm() + 1e-30))
            upd[kk] = (cos, float(um.norm() / uo.norm().clamp_min(1e-30)), float((uo - um).abs().max()), int(uo.numel()))
    assert nfrozen == 9 and len(upd) > 50                # two stems and fusion 0: a filter, gamma and beta each
    # ---- assert_k_step_parity, restated with its constants (loss_rtol 2e-2, min_cos 0.8, med_cos 0.985)
    for i, (lo, lm) in enumerate(losses):
        tol = 1e-4 if i == 0 else (2e-2 if i == 1 else 0.2)
        assert abs(lo - lm) <= tol * max(abs(lo), 1e-3), losses
    cosines = sorted(v[0] for v in upd.values())
    assert cosines[0] > 0.8 and float(np.median(cosines)) > 0.985, (cosines[:5], float(np.median(cosines)))
    for kk, (cos, ratio, mx, numel) in upd.items():
        lo_, hi_ = (0.9, 1.1) if numel > 64 else (0.75, 1.33)
        assert lo_ < ratio < hi_, (kk, ratio, numel)
        assert mx <= 3.2 * rate[kk] * k * 2, (kk, mx, rate[kk])


# ------------------------------------------------------------------ 5. defaults, config, refusals
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_empty_keywords_issue_todays_launches(optimizer):
    def record(**kw):
        m = _mini(backend=EmuGroupsBackend() if kw else EmuOptimBackend())
        tr = LaunchTrace(m.engine)
        st = TrainStep(m.engine, lr=1e-3, optimizer=optimizer, momentum=0.9 if optimizer == "sgd" else 0.0, **kw)
        assert state_present(m.engine) == [] and not st.opt.grouped and st.opt.segments is None and st.hp == ("lr_table" in kw)
        m.train()
        x, y = _batch()
        st(x[:, :5], x[:, 5:], y)
        pl = S.train_plan(m.engine)
        return dict(tr.take(), state=state_present(m.engine), ops=sorted(next(iter(st._cache.values()))["ops"]),
                    bwd=S.bwd_kinds(pl), marks=sorted(pl.grad_marks), frozen=m.engine.frozen_keys)
    assert record(param_groups=(), freeze=()) == record()
    base = dict(lr_table=[1e-3, 2e-3], clip_grad_norm=0.5)
    assert record(param_groups=[], freeze=[], **base) == record(**base)


def _cfg(name="slowfast-LHand", **model):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.INPUT_SIZE = 64
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.LR = 1e-2
    cfg.MODEL.MAX_EPOCH = 2
    cfg.NUM_CPU = 0
    for k, v in model.items():
        setattr(cfg.MODEL, k, v)
    return cfg


def test_config_keys_and_their_shapes(tmp_path):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.schedule import group_kwargs
    cfg = get_cfg()
    assert cfg.MODEL.PARAM_GROUPS == [] and cfg.MODEL.FREEZE == [] and group_kwargs(cfg) == {}
    y = tmp_path / "o.yaml"
    y.write_text("MODEL:\n  PARAM_GROUPS: [['@pretrained', 0.1], ['blocks.4.', 0.5, 0]]\n  FREEZE: ['blocks.0.']\n")
    cfg.merge_from_file(y)
    assert group_kwargs(cfg) == dict(param_groups=[("@pretrained", 0.1), ("blocks.4.", 0.5, 0.0)], freeze=["blocks.0."])
    assert group_kwargs(_cfg(FREEZE=["blocks.0."])) == dict(freeze=["blocks.0."])
    for bad in ([["blocks.1."]], [["blocks.1.", 0.1, 1.0, 2.0]], ["blocks.1."], [[0.1, "blocks.1."]], [["blocks.1.", "x"]],
                [["blocks.1.", True]], "blocks.1."):
        with pytest.raises(ValueError, match="PARAM_GROUPS"):
            group_kwargs(_cfg(PARAM_GROUPS=bad))
    for bad in ([0.5], "blocks.0.", [["blocks.0."]]):
        with pytest.raises(ValueError, match="FREEZE"):
            group_kwargs(_cfg(FREEZE=bad))


def test_optimizer_refuses_what_it_cannot_launch():
    eng = _mini(backend=EmuGroupsBackend()).engine
    for bad in (float("nan"), float("inf"), -0.5):
        with pytest.raises(ValueError, match="lr_mult"):
            Optimizer(eng, param_groups=[("blocks.1.", bad)])
        with pytest.raises(ValueError, match="wd_mult"):
            Optimizer(eng, param_groups=[("blocks.1.", 1.0, bad)])
    with pytest.raises(ValueError, match="param_groups entry"):
        Optimizer(eng, param_groups=[("blocks.1.",)])
    with pytest.raises(ValueError, match="64 selectors.*63"):
        Optimizer(eng, param_groups=[("blocks.1.", 1.0)] * 64)
    assert len(Optimizer(eng, param_groups=[("blocks.1.", 1.0)] * 63).group_decays) == 64
    with pytest.raises(ValueError, match="nothing trainable"):
        Optimizer(eng, freeze=["blocks."])
    with pytest.raises(ValueError, match="'blocks.9.' matches no key"):
        Optimizer(eng, freeze=["blocks.9."])
    with pytest.raises(ValueError, match="'layer1.' matches no key"):
        TrainStep(eng, lr=1e-3, param_groups=[("layer1.", 0.5)])
    with pytest.raises(ValueError, match="'@new'"):
        TrainStep(eng, lr=1e-3, freeze=["@new"])
    # more than 2048 segments: every second parameter tensor frozen leaves one segment per tensor
    many = _mini(backend=EmuGroupsBackend()).engine
    one = Optimizer(many, freeze=[many.param_tensors()[0][0]])
    assert 1 <= len(one.segments) <= 4
    old = Optimizer.MAX_SEGS
    try:
        Optimizer.MAX_SEGS = 3
        with pytest.raises(ValueError, match="segments: at most 3"):
            Optimizer(many, freeze=[k for k, _, _ in many.param_tensors()[0:16:2]])
    finally:
        Optimizer.MAX_SEGS = old
    assert state_present(eng) == [] and state_present(many) == []


def test_captured_step_refuses_groups_before_it_builds_anything():
    """the constructor path alone, with the engine's device type faked: nothing is captured, here or anywhere"""
    eng = _mini(backend=EmuGroupsBackend()).engine

    class Cuda:
        type = "cuda"
    real, eng.device = eng.device, Cuda()
    try:
        for kw in (dict(param_groups=[("blocks.1.", 0.1)]), dict(freeze=["blocks.0."]), dict(freeze=["blocks.9."])):
            with pytest.raises(ValueError, match="param_groups / freeze.*eager.*use_graph"):
                TrainStep(eng, lr=1e-3, use_graph=True, **kw)
    finally:
        eng.device = real
    assert state_present(eng) == [] and eng.adam_m is None and eng.frozen_keys == frozenset() and not eng._plans
    assert TrainStep(eng, lr=1e-3, use_graph=True, freeze=["blocks.0."]).opt.grouped      # on the CPU nothing is ever captured


# ------------------------------------------------------------------ 6. the trainers
def _trainer(which, tmp_path, **model):
    cfg = _cfg({"v2": "gesture-v2", "res2d": "res2d"}.get(which, "slowfast-LHand"), **model)
    cfg.CHALEARN.ROOT = str(tmp_path)
    be = EmuGroupsBackend()
    if which == "v2":
        tr = v2.SyntheticGesture(cfg, "train", num_videos=4, seed=1, h=48, w=64, min_box=8)
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
        return v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    return v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)


@pytest.mark.parametrize("which", ["v1", "v2", "res2d"])
def test_trainer_epoch_with_groups_and_a_frozen_stem(which, tmp_path, capsys):
    keys = (dict(FREEZE=["conv1.", "bn1."], PARAM_GROUPS=[["layer1.", 0.1]]) if which == "res2d" else
            dict(FREEZE=["blocks.0."], PARAM_GROUPS=[["blocks.1.", 0.1]]))
    t = _trainer(which, tmp_path, **keys)
    eng = t.model.engine
    assert t.step.opt.grouped and t.step.optimizer == ("sgd" if which == "v2" else "adam")
    keep = S.covered_mask(t.step.opt.segments, eng.arena_numel, eng.device)
    P0 = eng.P.data.clone()
    capsys.readouterr()
    loss, _ = t.train_epoch()
    out = capsys.readouterr().out
    assert loss == loss and 0.0 < loss < 20.0, loss
    assert S.same(eng.P.data[~keep], P0[~keep]) and 0 < int((~keep).sum())
    frozen_prefix = tuple(keys["FREEZE"])
    moved = {k: not S.same(eng.P.data[off:off + n], P0[off:off + n]) for k, off, n in eng.param_tensors()}
    assert not [k for k in moved if moved[k] and k.startswith(frozen_prefix)] and [k for k in moved if k.startswith(frozen_prefix)]
    # every other FILTER moved.  (The block-final gammas start at 0, so in the epoch's two steps the gradients inside the
    # blocks' branches are 0 and then tiny: Adam moves those tensors whatever their size, v2's SGD moves a BatchNorm weight
    # of 1 by less than half an ulp.)
    live = [k for k in moved if not k.startswith(frozen_prefix) and (which != "v2" or k.endswith(("conv.weight", "proj.weight")))]
    assert len(live) > 3 and all(moved[k] for k in live), [k for k in live if not moved[k]]
    for grp in (0, 1):
        gk = S.covered_mask([s_ for s_ in t.step.opt.segments if s_[2] == grp], eng.arena_numel, eng.device)
        assert bool(gk.any()) and not S.same(eng.P.data[gk], P0[gk]), grp
    rates = t.step.last_lrs()
    assert len(rates) == 2 and rates[1] == float(np.float32(0.1 * 1e-2)) and rates[0] == float(np.float32(1e-2))
    assert f"lr: [{rates[0]:.6g}, {rates[1]:.6g}]" in out, out
    pl = S.train_plan(eng)
    assert not [k for k in S.bwd_kinds(pl) if k[0] == "stem_wgrad"] and pl.tail_cut is None


def test_trainer_defaults_pass_no_group_keyword(tmp_path, capsys):
    t = _trainer("v1", tmp_path)
    assert t._group_kwargs() == {} and not t.step.opt.grouped and not t.step.hp and t.model.engine.frozen_keys == frozenset()
    t.train_epoch()
    assert "lr:" not in capsys.readouterr().out


def test_res2d_with_the_torch_backend_refuses_the_keys(tmp_path):
    for keys in (dict(FREEZE=["conv1."]), dict(PARAM_GROUPS=[["layer1.", 0.1]])):
        cfg = _cfg("res2d", RES2D_BACKEND="torch", **keys)
        tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
        te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
        with pytest.raises(ValueError, match="PARAM_GROUPS / FREEZE.*res2d.*torch"):
            v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuGroupsBackend())


# ------------------------------------------------------------------ 7. two ranks over gloo
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    from video_classification_amd import arch, dist as sdist
    from video_classification_amd.slowfast import SlowFast
    r, w, _ = sdist.init_process_group_from_env("gloo")
    assert (r, w) == (rank, world)
    spec = arch.ref_spec(num_class=5, depth=18, head_pool_kernels=((2, 1, 1), (2, 1, 1)))
    m = SlowFast(spec, dtype=torch.float32, device="cpu", backend=EmuGroupsBackend(), seed=3)
    eng = m.engine
    S.mark_fresh(eng)
    g = torch.Generator().manual_seed(100)
    clips = torch.randn(world * 2, 4, 21, 32, 32, generator=g)
    labels = torch.randint(0, 5, (world * 2,), generator=g)
    idx = sdist.shard_indices(world * 2, rank, world, epoch_seed=0, shuffle=False)
    x = clips[idx].permute(0, 2, 1, 3, 4)
    m.train()
    P0 = eng.P.data.clone()
    red = sdist.GradReducer(eng.G, bucket_mb=0.25)
    step = TrainStep(eng, lr=1e-2, lr_table=S.TABLE, weight_decay=0.1, decay_mode="decoupled", param_groups=S.GROUPS,
                     freeze=S.FREEZE, reducer=red, overlap_segments=4)
    assert step.world == world and step.segmented
    for _ in range(2):
        step(x[:, 0:5], x[:, 5:20], labels[idx])
    pl = S.train_plan(eng)
    torch.save({"P": eng.P.data.clone(), "G": eng.G.clone(), "m": eng.adam_m.clone(), "P0": P0, "reduced": list(red.reduced),
                "marked": S.marked_mask(pl, eng.arena_numel, eng.device), "segments": step.opt.segments,
                "marks": sorted(r for _, r in pl.grad_marks)}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_grouped_step_gloo(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    for k in ("P", "G", "m", "P0"):
        assert S.same(a[k], b[k]), k
    n = a["P"].numel()
    keep = S.covered_mask(a["segments"], n, "cpu")
    assert S.same(a["P"][~keep], a["P0"][~keep]) and not S.same(a["P"][keep], a["P0"][keep])
    # the reducer exchanged exactly the ranges of the writers left, once each per step: none of a dropped writer
    cover = torch.zeros(n, dtype=torch.int32)
    for off, cnt in a["reduced"]:
        cover[off:off + cnt] += 1
    per_step = cover[a["marked"]]
    assert int(per_step.min()) == int(per_step.max()) and int(per_step.min()) >= 1
    assert not bool(cover[~a["marked"]].any()) and bool((~a["marked"]).any())
    assert not bool((keep & ~a["marked"]).any())
