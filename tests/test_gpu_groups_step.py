"""Parameter groups and frozen layers from the train step up on an MI355X, eager steps only.  The
grouped step against HipBackend's own sfk_adam_hp / sfk_sgd_hp on every segment's slices within ONE run (filter gradients use
atomics, so two runs are never compared: tests/groups_step_ref.py, as tests/ref_ema.check_route does), bf16 and fp32, on the
depth-18 SlowFast of tests/test_gpu_ema.py (2 clips of 4 x 64 x 64: the smallest shapes at which every tile path of the step
still runs) and on the res2d engine mini; the pruned train plans with deterministic filter gradients against the unpruned
engine; one epoch of each trainer with the keys set; the use_graph refusal, by constructing only.  No TrainStep is captured.
tests/test_groups_step_cpu.py runs the same checks on the emulated backend and shows that wrong launches fail them."""
import pytest
import torch

import groups_step_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    return HipBackend()


def _mini(dtype, options=None, depth=18):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=depth, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=dtype, device=DEV, options=options)


def _clips(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(2, 4, 7, 64, 64, generator=g).permute(0, 2, 1, 3, 4).to(DEV).to(dtype)
    return clips[:, 0:5].contiguous(), clips[:, 5:7].contiguous(), torch.tensor([1, 4], device=DEV)


# ------------------------------------------------------------------ the grouped step, bit for bit within one run
ROUTES = {
    # the fast stem trains, so the eager default splits the update beside its filter gradient: adam_main + adam_tail
    "split": (dict(weight_decay=0.1, decay_mode="decoupled"), ["blocks.0.multipathway_blocks.0."]),
    "frozen-stems": (dict(weight_decay=0.1, decay_mode="decoupled"), S.FREEZE),
    "clip": (dict(weight_decay=0.1, decay_mode="decoupled", clip_grad_norm=1.0), S.FREEZE),
    "sgd": (dict(optimizer="sgd", momentum=0.9, weight_decay=0.1, decay_mode="l2"), S.FREEZE),
}


@DTYPES
@pytest.mark.parametrize("route", list(ROUTES))
def test_grouped_step_is_the_hp_kernel_on_every_segment(hip, route, dtype):
    from video_classification_amd.train import TrainStep
    kw, freeze = ROUTES[route]
    m = _mini(dtype)
    eng = m.engine
    S.mark_fresh(eng)
    m.train()
    step = TrainStep(eng, lr=1e-3, lr_table=S.TABLE, param_groups=S.GROUPS, freeze=freeze, **kw)
    xs, xf, y = _clips(dtype)
    vs = S.check_grouped_steps(step, lambda: step(xs, xf, y), hip, 4)
    ops = next(iter(step._cache.values()))["ops"]
    pl = S.train_plan(eng)
    print("ops", sorted(ops), "segments", len(step.opt.segments), "rates", step.last_lrs())
    assert ("adam_main" in ops and "adam_tail" in ops and pl.tail_cut is not None) == (route == "split")
    assert ("grad_norm" in ops) == (route == "clip")
    assert len([k for k in S.bwd_kinds(pl) if k[0] == "stem_wgrad"]) == (1 if route == "split" else 0)
    assert {grp for _, _, grp, _ in step.opt.segments} == {0, 1, 2} and len(step.last_lrs()) == 3
    S.report(vs)


def test_grouped_step_on_the_res2d_engine(hip):
    from video_classification_amd.slowfast import resnet50_2d_engine
    from video_classification_amd.train import TrainStep
    m = resnet50_2d_engine(num_class=7, clip_len=2, crop=64, dtype=torch.bfloat16, device=DEV, depth=18)
    eng = m.engine
    m.train()
    step = TrainStep(eng, lr=1e-3, lr_table=S.TABLE, weight_decay=0.1, decay_mode="decoupled",
                     param_groups=[("layer1.", 0.1), ("fc.", 0.5, 0.0)], freeze=["conv1.", "bn1."])
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 10, 64, 64, generator=g).to(DEV).to(torch.bfloat16)
    y = torch.tensor([1, 4], device=DEV)
    vs = S.check_grouped_steps(step, lambda: step(x, None, y), hip, 3)
    pl = S.train_plan(eng)
    assert not [k for k in S.bwd_kinds(pl) if k[0] == "stem_wgrad" or S.under(k[1], ("conv1", "bn1"))]
    S.report(vs)


# ------------------------------------------------------------------ the pruned plans
CONV_A = "blocks.2.multipathway_blocks.0.res_blocks.0.branch2.conv_a"
PRUNED = {"stems": ["blocks.0."], "through-res3": ["blocks.0.", "blocks.1.", "blocks.2."], "one-filter": [CONV_A + ".weight"]}


def _one_step(dtype, freeze, depth=18):
    from video_classification_amd.engine import EngineOptions
    from video_classification_amd.train import TrainStep
    m = _mini(dtype, EngineOptions(deterministic_wgrad=True), depth)
    m.train()
    for L in m.engine.layers:                            # the block-final gammas start at 0, which zeroes every gradient inside
        if L.cb.zero_init_gamma:                         # the blocks' branches: give the dropped writers something to write
            m.engine.P.data[L.g_off:L.g_off + L.c] = 0.5
    step = TrainStep(m.engine, lr=1e-3, freeze=freeze) if freeze else TrainStep(m.engine, lr=1e-3)
    xs, xf, y = _clips(dtype)
    step(xs, xf, y)
    torch.cuda.synchronize()
    return m.engine, step, S.train_plan(m.engine)


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def unpruned(request):
    eng, _, pl = _one_step(request.param, ())
    return dict(dtype=request.param, G=eng.G.clone(), kinds=S.bwd_kinds(pl), joins=S.joins(pl))


@pytest.mark.parametrize("case", list(PRUNED))
def test_frozen_set_prunes_the_train_plan(unpruned, case):
    freeze = PRUNED[case]
    eng, step, pl = _one_step(unpruned["dtype"], freeze)
    kinds = S.bwd_kinds(pl)
    if case == "one-filter":
        assert kinds == [k for k in unpruned["kinds"] if k != ("conv_wgrad", CONV_A)] and len(kinds) == len(unpruned["kinds"]) - 1
    else:
        assert not [k for k in kinds if k[0] == "stem_wgrad" or S.under(k[1], freeze)] and pl.tail_cut is None
        it = iter(unpruned["kinds"])
        assert all(k in it for k in kinds) and len(kinds) < len(unpruned["kinds"])
    assert S.joins(pl)[-3:] == unpruned["joins"][-3:] == [(0, 1), (0, 2), (0, 3)]
    # G after step 1: bit for bit the unpruned engine's on every range a writer is left for, outside the two stems' filters
    # (stem_wgrad flushes with atomics under every switch); zero where the writer was dropped
    marked = S.marked_mask(pl, eng.arena_numel, eng.device)
    stems = torch.zeros_like(marked)
    for st in eng.wiring.stems:
        L = eng._layers[st.conv_key]
        stems[L.w_off:L.w_off + L.w_numel] = True
    cmp = marked & ~stems
    assert S.same(eng.G[cmp], unpruned["G"][cmp]) and bool(eng.G[cmp].any())
    assert not bool(eng.G[~marked].any()) and bool(unpruned["G"][~marked].any())
    keep = S.covered_mask(step.opt.segments, eng.arena_numel, eng.device)
    assert not bool((keep & ~marked).any())


@DTYPES
def test_the_cut_falls_inside_a_stage_at_two_blocks_per_stage(dtype):
    """depth 26, two blocks per stage: res4's second fast block is the last trainable unit, its first one is not emitted"""
    fast_b0 = "blocks.3.multipathway_blocks.1.res_blocks.0."
    freeze = ["blocks.0.", "blocks.1.", "blocks.2.", fast_b0]
    base, _, bpl = _one_step(dtype, (), 26)
    eng, step, pl = _one_step(dtype, freeze, 26)
    kinds, all_kinds = S.bwd_kinds(pl), S.bwd_kinds(bpl)
    kept = fast_b0.replace("res_blocks.0.", "res_blocks.1.")
    assert [k for k in all_kinds if S.under(k[1], [fast_b0])] and not [k for k in kinds if S.under(k[1], freeze)]
    assert [k for k in kinds if S.under(k[1], [kept])] == [k for k in all_kinds if S.under(k[1], [kept])]
    it = iter(all_kinds)
    assert all(k in it for k in kinds) and len(kinds) < len(all_kinds)
    marked = S.marked_mask(pl, eng.arena_numel, eng.device)
    assert S.same(eng.G[marked], base.G[marked]) and bool(eng.G[marked].any())        # (the stems are frozen: no atomics left)
    assert not bool(eng.G[~marked].any()) and bool(base.G[~marked].any())
    keep = S.covered_mask(step.opt.segments, eng.arena_numel, eng.device)
    assert not bool((keep & ~marked).any())


# ------------------------------------------------------------------ the trainers
@pytest.mark.parametrize("which,ema", [("v1", False), ("v2", False), ("v1", True)], ids=["v1", "v2", "v1-ema"])
def test_trainer_epoch_with_the_keys_set(which, ema, tmp_path, capsys):
    from test_ema_cpu import make_trainer
    extra = dict(EMA_DECAY=0.9, EMA_WARMUP=True) if ema else {}
    t = make_trainer(which, tmp_path, device=DEV, DTYPE="bf16", FREEZE=["blocks.0."], PARAM_GROUPS=[["blocks.1.", 0.1]], **extra)
    eng = t.model.engine
    assert t.step.opt.grouped and (t.step.ema is not None) == ema and t.step.optimizer == ("sgd" if which == "v2" else "adam")
    keep = S.covered_mask(t.step.opt.segments, eng.arena_numel, eng.device)
    P0 = eng.P.data.clone()
    capsys.readouterr()
    loss, _ = t.train_epoch()
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    assert loss == loss and 0.0 < loss < 20.0, loss
    assert S.same(eng.P.data[~keep], P0[~keep]) and bool((~keep).any())
    for grp in (0, 1):
        gk = S.covered_mask([s_ for s_ in t.step.opt.segments if s_[2] == grp], eng.arena_numel, eng.device)
        assert bool(gk.any()) and not S.same(eng.P.data[gk], P0[gk]), grp
    rates = t.step.last_lrs()
    assert len(rates) == 2 and f"lr: [{rates[0]:.6g}, {rates[1]:.6g}]" in out, out
    if ema:                                              # frozen elements average to themselves
        assert int(eng.ema_step[0]) == t.step.steps and S.same(eng.ema_P[~keep], P0[~keep])
        assert not S.same(eng.ema_P[keep], P0[keep])
    pl = S.train_plan(eng)
    assert not [k for k in S.bwd_kinds(pl) if k[0] == "stem_wgrad"] and pl.tail_cut is None


# ------------------------------------------------------------------ the refusal (constructed, never captured)
def test_captured_step_refuses_groups_before_it_builds_anything():
    from video_classification_amd.train import TrainStep
    eng = _mini(torch.float32).engine
    for kw in (dict(param_groups=[("blocks.1.", 0.1)]), dict(freeze=["blocks.0."])):
        with pytest.raises(ValueError, match="param_groups / freeze.*eager.*use_graph"):
            TrainStep(eng, lr=1e-3, use_graph=True, **kw)
    assert eng.adam_m is None and eng.frozen_keys == frozenset() and not eng._plans
    assert not TrainStep(eng, lr=1e-3, use_graph=True, param_groups=(), freeze=()).opt.grouped
