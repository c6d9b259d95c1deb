"""include/sfk_optim.h without a GPU: the float64 restatements (tests/optim_ref64.py) against torch's own optimizers,
clip_grad_norm_ and schedulers; the honest-float32 emulation (tests/emu_optim.py) inside the bounds and its mutants outside
them; TrainStep's new keywords on the emulated backend against torch; the ABI of the new header."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import head_ref64 as H
import optim_ref64 as O
from emu_optim import EmuOptimBackend
from ref64 import F64, compare, ulp_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
f32 = H.f32
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
TABLE = [f32(x) for x in O.LR_TABLE]


# ------------------------------------------------------------------ the float64 restatements are torch's, in float64
def _inputs64(count=257, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(count, generator=g, dtype=F64) for _ in range(2)]


def _ok(v):
    assert v.ok, v


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("clip", [False, True])
def test_adam_ref64_is_torch_adam_and_adamw(mode, clip):
    p0, _ = _inputs64()
    count, dc = p0.numel(), p0.numel()
    wd = {"none": 0.0, "l2": O.WD, "decoupled": O.WD}[mode]
    tp = p0.clone().requires_grad_(True)
    cls = torch.optim.AdamW if mode == "decoupled" else torch.optim.Adam
    opt = cls([tp], lr=TABLE[0], betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros(count, dtype=F64), torch.zeros(count, dtype=F64)
    gen = torch.Generator().manual_seed(3)
    for s in range(1, 7):                                         # past the end of the table: the last rate holds
        g = torch.randn(count, generator=gen).double()          # float32 values: what the norm kernel is given
        coef = None
        tp.grad = g.clone()
        if clip:
            norm, c = O.grad_norm_ref(g, 1.0, 2.0)
            tn = torch.nn.utils.clip_grad_norm_([tp], 2.0)
            _ok(H.ElemOnly(compare("norm", tn.reshape(1), norm.reshape(1), norm.reshape(1), 1, F32, "map_f32")))
            coef = float(c)
        opt.param_groups[0]["lr"] = TABLE[O.table_index(s, len(TABLE))]
        opt.step()
        # the restatement takes the coefficient as the float32 the kernel reads: feed it the double through gscale instead
        r = O.adam_hp_ref(p, g, m, v, s, TABLE, B1, B2, EPS, 1.0, wd, mode, dc, None) if coef is None else \
            O.adam_hp_ref(p, g * coef, m, v, s, TABLE, B1, B2, EPS, 1.0, wd, mode, dc, None)
        st = opt.state[tp]
        _ok(compare(f"m step {s}", st["exp_avg"], r["m"], r["a_m"], 2, F32, "map_f32"))
        _ok(compare(f"v step {s}", st["exp_avg_sq"], r["v"], r["a_v"], 2, F32, "map_f32"))
        _ok(H.compare_p(f"p step {s}", tp.detach(), r))
        assert float((tp.detach() - r["p"]).abs().max()) < 1e-12
        p, m, v = r["p"], r["m"], r["v"]


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (O.SGD_MOM, False), (O.SGD_MOM, True)])
def test_sgd_ref64_is_torch_sgd_with_weight_decay(momentum, nesterov):
    p0, _ = _inputs64(seed=1)
    count = p0.numel()
    mom, damp = f32(momentum), (0.0 if nesterov else 0.25)       # (1 - 0.25 is exact in float32, as the ABI forms it)
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=TABLE[0], momentum=mom, dampening=damp, nesterov=nesterov, weight_decay=O.WD, foreach=False)
    p, buf = p0.clone(), torch.zeros(count, dtype=F64)
    gen = torch.Generator().manual_seed(4)
    for s in range(1, 7):
        g = torch.randn(count, generator=gen, dtype=F64)
        tp.grad = g.clone()
        opt.param_groups[0]["lr"] = TABLE[O.table_index(s, len(TABLE))]
        opt.step()
        r = O.sgd_hp_ref(p, g, buf, s, TABLE, mom, damp, nesterov, 1.0, O.WD, "l2", count, None)
        _ok(compare(f"p step {s}", tp.detach(), r["p"], r["a_p"], 4, F32, "map_f32"))
        assert float((tp.detach() - r["p"]).abs().max()) < 1e-12
        if momentum != 0:
            assert float((opt.state[tp]["momentum_buffer"] - r["buf"]).abs().max()) < 1e-12
            buf = r["buf"]
        p = r["p"]


def test_norm_ref64_is_torch_clip_grad_norm():
    gen = torch.Generator().manual_seed(5)
    for max_norm in (0.5, 1e3):                                   # clipped, and clamped at 1
        ps = [torch.zeros(n, dtype=F64, requires_grad=True) for n in (7, 130, 1)]
        for p in ps:
            p.grad = torch.randn(p.numel(), generator=gen).double()     # float32 values: what the kernel is given
        flat = torch.cat([p.grad.clone() for p in ps])
        norm, c = O.grad_norm_ref(flat, 1.0, max_norm)
        n2, clipped = O.clip_grad_norm_ref([p.grad.clone() for p in ps], max_norm)
        tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(float(tn) - float(norm)) <= 1e-12 * float(norm) and abs(float(n2) - float(norm)) <= 1e-12 * float(norm)
        assert float(c) <= 1.0 and (float(c) == 1.0) == (max_norm > float(norm))
        got = torch.cat([p.grad for p in ps])
        assert float((got - flat * c).abs().max()) <= 1e-9 * float(flat.abs().max())   # (the restatement's 1e-6 is float32's)
        assert float((got - torch.cat(clipped)).abs().max()) <= 1e-15
    for kind, want in (("inf", (math.inf, 0.0)), ("nan", (math.nan, math.nan))):
        p = torch.zeros(9, dtype=F64, requires_grad=True)
        p.grad = torch.ones(9, dtype=F64)
        p.grad[4] = float(kind)
        norm, c = O.grad_norm_ref(p.grad, 1.0, 1.0)
        tn = torch.nn.utils.clip_grad_norm_([p], 1.0)
        for got, ref, w in ((float(tn), float(norm), want[0]), (None, float(c), want[1])):
            assert (math.isnan(ref) and math.isnan(w)) or ref == w
            assert got is None or (math.isnan(got) and math.isnan(w)) or got == w


# ------------------------------------------------------------------ the schedule tables are torch's schedulers, step by step
def _torch_rates(make, total):
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=LR0)
    sched = make(opt)
    out = []
    for _ in range(total):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


LR0 = 5e-4


def _same_at_float32(table, rates):
    assert len(table) == len(rates)
    t, r = torch.tensor(table, dtype=F64), torch.tensor(rates, dtype=F64)
    assert bool(((t.float().double() - r.float().double()).abs() <= ulp_out(r, F32)).all()), (table[:8], rates[:8])


@pytest.mark.parametrize("warmup,total,lr_min", [(5, 40, 0.0), (1, 17, 1e-5), (8, 9, 1e-6)])
def test_cosine_table_is_sequential_linear_then_cosine(warmup, total, lr_min):
    import warnings
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    from video_classification_amd.schedule import lr_schedule

    def make(opt):
        return SequentialLR(opt, [LinearLR(opt, start_factor=1.0 / warmup, end_factor=1.0, total_iters=warmup),
                                  CosineAnnealingLR(opt, T_max=total - warmup, eta_min=lr_min)], milestones=[warmup])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rates = _torch_rates(make, total)
    table = lr_schedule("cosine", LR0, 1, total, warmup_steps=warmup, lr_min=lr_min)
    _same_at_float32(table, rates)
    assert table[0] == pytest.approx(LR0 / warmup) and table[warmup] == LR0 and min(table[warmup:]) > lr_min


def test_cosine_table_without_warmup_and_constant_and_multistep():
    from torch.optim.lr_scheduler import CosineAnnealingLR, MultiStepLR
    from video_classification_amd.schedule import lr_schedule
    table = lr_schedule("cosine", LR0, 3, 7, lr_min=1e-6)
    _same_at_float32(table, _torch_rates(lambda o: CosineAnnealingLR(o, T_max=21, eta_min=1e-6), 21))
    assert lr_schedule("constant", LR0, 3, 7) == [LR0] * 21
    spe, epochs, ms = 3, 9, [2, 5, 6]
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=LR0)
    sched = MultiStepLR(opt, milestones=ms, gamma=0.3)
    rates = []
    for _ in range(epochs):
        for _ in range(spe):
            rates.append(opt.param_groups[0]["lr"])
            opt.step()
        sched.step()
    _same_at_float32(lr_schedule("multistep", LR0, epochs, spe, milestones=ms, gamma=0.3), rates)
    with pytest.raises(ValueError):
        lr_schedule("poly", LR0, 1, 1)
    with pytest.raises(ValueError):
        lr_schedule("cosine", LR0, 1, 4, warmup_steps=4)


def test_config_keys_default_to_no_keywords():
    from video_classification_amd.config import get_cfg
    from video_classification_amd.schedule import optim_kwargs
    cfg = get_cfg()

    def never():
        raise AssertionError("the constant schedule must not ask for the epoch's length")
    assert optim_kwargs(cfg, never) == {}
    cfg.MODEL.LR_SCHEDULE, cfg.MODEL.LR_WARMUP_STEPS, cfg.MODEL.MAX_EPOCH = "cosine", 3, 2
    cfg.MODEL.WEIGHT_DECAY, cfg.MODEL.CLIP_GRAD_NORM = 0.05, 1.5
    kw = optim_kwargs(cfg, lambda: 10)
    assert len(kw["lr_table"]) == 20 and kw["decay_mode"] == "decoupled" and kw["decay_scope"] == "weights"
    assert kw["weight_decay"] == 0.05 and kw["clip_grad_norm"] == 1.5
    for key, bad in (("LR_SCHEDULE", "poly"), ("WEIGHT_DECAY_MODE", "adamw"), ("WEIGHT_DECAY_SCOPE", "bias"), ("CLIP_GRAD_NORM", -1.0)):
        c2 = cfg.clone()
        c2.MODEL[key] = bad
        with pytest.raises(ValueError):
            optim_kwargs(c2, 10)


# ------------------------------------------------------------------ the honest float32 emulation is inside the bounds
SMALL = O.COUNTS


def _run_table(be, count, kernel):
    vs = []
    for dc, s0, off, sh, clip, mi in O.hp_case_table(count):
        if kernel == "adam":
            vs += O.check_adam_hp(be, "cpu", count, dc, s0, off, sh, clip, O.MODES[mi])
        else:
            vs += O.check_sgd_hp(be, "cpu", count, dc, s0, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2))
    return vs


@pytest.mark.parametrize("count", SMALL)
def test_emu_optimizer_updates_are_inside_the_bounds(count):
    be = EmuOptimBackend()
    bad = H.failures(_run_table(be, count, "adam") + _run_table(be, count, "sgd"))
    assert not bad, bad[:5]


def test_emu_every_option_crossed_at_one_count():
    be, bad = EmuOptimBackend(), []
    for off, sh, clip, mi in O.hp_cross_table():
        bad += H.failures(O.check_adam_hp(be, "cpu", 1025, 5, 1, off, sh, clip, O.MODES[mi]))
        bad += H.failures(O.check_sgd_hp(be, "cpu", 1025, 5, 1, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2)))
        bad += H.failures(O.check_sgd_hp(be, "cpu", 1025, 5, 1, off, sh, clip, O.MODES[mi % 2], momentum=0.0))
    assert not bad, bad[:5]


def _norm_cases(be, count):
    vs = []
    for kind in ("randn", "zero", "inf", "nan"):
        for off in (0, 1):
            vs += O.check_grad_norm(be, "cpu", count, kind, off)
    vs += O.check_grad_norm(be, "cpu", count, "randn", 0, gscale=1.0, max_norm=1e6)      # clamped at 1
    return vs


@pytest.mark.parametrize("count", SMALL)
def test_emu_grad_norm_is_inside_the_bounds(count):
    bad = H.failures(_norm_cases(EmuOptimBackend(), count))
    assert not bad, bad[:5]


def test_emu_split_pair_equals_the_single_launch():
    be, bad = EmuOptimBackend(), []
    for count, dc in ((4099, 2048), (1025, 5)):
        for cut in sorted({c for c in (4, dc - 4 - dc % 4, dc - dc % 4, dc - dc % 4 + 4, count - count % 4 - 4) if 0 < c < count}):
            for mode in O.MODES:
                bad += H.failures(O.check_adam_hp_split(be, "cpu", count, cut, dc, 1, mode))
    assert not bad, bad[:5]


def test_grad_norm_rows_depend_on_count_only():
    be = EmuOptimBackend()
    assert [be.grad_norm_parts(c) for c in (1, 4096, 4097, 2048 * 4096, O.BIG, 1 << 40)] == [1, 1, 2, 2048, 2048, 2048]
    with pytest.raises(ValueError):
        be.grad_norm_parts(0)


# ------------------------------------------------------------------ the mutants are outside them
def _mutant(**attrs):
    return type("M", (EmuOptimBackend,), attrs)()


def _rejected(be, count, kernel, pick=lambda case: True):
    """per case of the table: does the mutant fail it?"""
    out = []
    for case in filter(pick, O.hp_case_table(count)):
        dc, s0, off, sh, clip, mi = case
        if kernel == "adam":
            vs = O.check_adam_hp(be, "cpu", count, dc, s0, off, sh, clip, O.MODES[mi])
        else:
            vs = O.check_sgd_hp(be, "cpu", count, dc, s0, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2))
        out.append(bool(H.failures(vs)))
    return out


def _decays(kernel):
    return (lambda c: c[5] != 0 and c[0] > 0) if kernel == "adam" else (lambda c: c[5] % 2 == 1 and c[0] > 0)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_decay_after_the_update_is_rejected(kernel):
    be = _mutant(decay_after_update=True)
    for count in (5, 1025):
        # (where one or five entries decay, AdamW's mutation shows only through their own dp * lr * wd, which an entry with a
        # gradient near zero hides: the cases in which the whole slice, or all but its last entry, decays must all refuse it)
        got = _rejected(be, count, kernel, lambda c: _decays(kernel)(c) and c[0] >= count - 1)
        assert got and all(got), (count, got)
    assert not any(_rejected(be, 1025, kernel, lambda c: not _decays(kernel)(c) and c[0] == 0))


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_decay_of_the_complement_range_is_rejected(kernel):
    be = _mutant(decay_wrong_range=True)
    mode_on = (lambda c: c[5] != 0) if kernel == "adam" else (lambda c: c[5] % 2 == 1)
    for count in (5, 1025):
        got = _rejected(be, count, kernel, mode_on)
        assert got and all(got), (count, got)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_table_index_off_by_one_is_rejected(kernel):
    be = _mutant(table_off=1)
    inside = lambda c: c[1] + 1 < len(O.LR_TABLE)                 # (at and past the last entry both clamp to it)
    got = _rejected(be, 1025, kernel, inside)
    assert got and all(got), got
    assert not any(_rejected(be, 1025, kernel, lambda c: not inside(c)))


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_table_without_the_clamp_at_its_length_is_rejected(kernel):
    be = _mutant(table_unclamped=True)
    past = lambda c: c[1] + 1 > len(O.LR_TABLE)
    got = _rejected(be, 1025, kernel, past)
    assert got and all(got), got
    assert not any(_rejected(be, 1025, kernel, lambda c: not past(c)))


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_without_the_last_count_mod_4_elements_is_rejected(kernel):
    be = _mutant(skip_mod4_tail=True)
    for count in (1, 3, 5, 1023, 1025, 4099):
        assert all(_rejected(be, count, kernel)), count
    assert not any(_rejected(be, 1024, kernel))
    for count in (3, 4099):
        assert H.failures(O.check_grad_norm(be, "cpu", count))
    assert not H.failures(O.check_grad_norm(be, "cpu", 1024))


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_mutant_that_stops_at_the_grid_cap_is_rejected(kernel):
    """(the cap of the emulation is lowered to 4096 elements, so that the count above it stays small on the CPU; the GPU test
    runs the real cap)"""
    be = _mutant(grid_cap=4096)
    assert all(_rejected(be, 4099, kernel))
    assert not any(_rejected(be, 1025, kernel))
    assert H.failures(O.check_grad_norm(be, "cpu", 4099)) and not H.failures(O.check_grad_norm(be, "cpu", 1025))


def test_mutant_coefficient_not_clamped_at_one_is_rejected():
    be = _mutant(coef_unclamped=True)
    for count in SMALL:
        assert H.failures(O.check_grad_norm(be, "cpu", count, "randn", 0, gscale=1.0, max_norm=1e6)), count
        assert H.failures(O.check_grad_norm(be, "cpu", count, "zero")), count
        assert not H.failures(O.check_grad_norm(be, "cpu", count, "randn"))         # below 1 the clamp does nothing


def test_mutant_norm_before_grad_scale_is_rejected():
    be = _mutant(norm_before_scale=True)
    for count in SMALL:
        assert H.failures(O.check_grad_norm(be, "cpu", count, "randn", 0, gscale=0.5)), count
        assert not H.failures(O.check_grad_norm(be, "cpu", count, "randn", 0, gscale=1.0))


# ------------------------------------------------------------------ TrainStep on the emulated backend
class Recorder(EmuOptimBackend):
    """notes the optimizer-side launches in the order they run"""

    def __init__(self):
        self.ran = []

    def _note(self, name, run):
        def wrapped(stream):
            self.ran.append(name)
            run(stream)
        return wrapped


for _n in ("adam", "sgd", "adam_hp", "sgd_hp", "grad_norm"):
    def _make(name):
        def method(self, *a, **k):
            return self._note(name, getattr(EmuOptimBackend, name)(self, *a, **k))
        return method
    setattr(Recorder, _n, _make(_n))


def _mini(seed=0, backend=None, scale=1.0):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    m = SlowFast(spec, dtype=torch.float32, device="cpu", backend=backend or EmuOptimBackend(), seed=seed)
    if scale != 1.0:
        m.engine.P.data.mul_(scale)
    return m


def _batches(k, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 7, 4, 64, 64, generator=g), torch.randint(0, 7, (2,), generator=g)) for _ in range(k)]


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_default_keywords_issue_the_same_launches_as_before(optimizer):
    from video_classification_amd.train import TrainStep
    for kw in ({}, dict(weight_decay=0.0, decay_mode="l2", clip_grad_norm=0.0), dict(weight_decay=0.3, decay_mode="none")):
        be = Recorder()
        m = _mini(backend=be)
        st = TrainStep(m.engine, lr=1e-3, optimizer=optimizer, momentum=0.9 if optimizer == "sgd" else 0.0, **kw)
        assert not st.hp and st.lr_table is None and st.grad_norm is None
        m.train()
        for x, y in _batches(2):
            st(x[:, :5], x[:, 5:], y)
        assert be.ran == [optimizer, optimizer]
        assert m.engine.grad_norm is None
        ops = next(iter(st._cache.values()))["ops"]
        assert sorted(ops) == ["adam", "loss", "zero_grad", "zero_loss"]


def test_trainstep_keyword_validation():
    from video_classification_amd.train import TrainStep
    m = _mini()
    for kw in (dict(decay_mode="adamw"), dict(decay_scope="bias"), dict(weight_decay=-1.0), dict(clip_grad_norm=-1.0),
               dict(optimizer="sgd", weight_decay=0.1, decay_mode="decoupled"), dict(lr_table=[])):
        with pytest.raises(ValueError):
            TrainStep(m.engine, lr=1e-3, **kw)


BASE_LR, WD, MAX_NORM, WARMUP, TOTAL = 1e-4, 0.1, 0.5, 2, 6
P_SCALE = 0.25      # every |parameter| below 0.5: the comparison's 1e-7 is then more than three units in the last place


def _torch_side(eng, make_opt):
    """the arena as two torch parameters -- the decayed prefix and the rest -- under torch's optimizer, clip_grad_norm_ and
    SequentialLR(LinearLR, CosineAnnealingLR), in float64: torch's float32 clip_grad_norm_ sums 10^7 squares in float32 and is
    itself 3e-5 off the norm, which would be the reference's error and not the step's"""
    import warnings
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    cut = eng.fc_b_off
    pw = eng.P.data[:cut].double().clone().requires_grad_(True)
    pr = eng.P.data[cut:].double().clone().requires_grad_(True)
    opt = make_opt([dict(params=[pw], weight_decay=WD), dict(params=[pr], weight_decay=0.0)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = SequentialLR(opt, [LinearLR(opt, start_factor=1.0 / WARMUP, end_factor=1.0, total_iters=WARMUP),
                                   CosineAnnealingLR(opt, T_max=TOTAL - WARMUP, eta_min=0.0)], milestones=[WARMUP])
    return pw, pr, opt, sched


def _three_steps_against_torch(optimizer, make_opt, step_kw, state_of):
    """three steps of the schedule, each against torch from the same state: after a step is compared, the engine takes
    torch's parameters and optimizer state (rounded to float32), as tests/test_gpu_v2.py does for sfk_sgd -- Adam's update
    m / (sqrt(v) + eps) of an entry whose gradient is near zero amplifies a last-place difference of the previous step beyond
    any fixed absolute tolerance, which says nothing about the launch under test.  The step counter, and with it the table
    entry and the bias corrections, runs on."""
    import warnings
    from video_classification_amd.schedule import lr_schedule
    from video_classification_amd.train import TrainStep
    be = Recorder()
    a, b = _mini(backend=be, scale=P_SCALE), _mini(scale=P_SCALE)
    assert torch.equal(a.engine.P.data, b.engine.P.data)
    table = lr_schedule("cosine", BASE_LR, 1, TOTAL, warmup_steps=WARMUP)
    sa = TrainStep(a.engine, lr=BASE_LR, optimizer=optimizer, lr_table=table, clip_grad_norm=MAX_NORM, **step_kw)
    sb = TrainStep(b.engine, lr=0.0)                          # the gradient only (Adam with lr 0 leaves P as it is)
    pw, pr, opt, sched = _torch_side(b.engine, make_opt)
    cut = b.engine.fc_b_off
    a.train(); b.train()
    clipped = 0
    for k, (x, y) in enumerate(_batches(3)):
        la = float(sa(x[:, :5], x[:, 5:], y))
        lb = float(sb(x[:, :5], x[:, 5:], y))
        assert la == lb
        pw.grad, pr.grad = b.engine.G[:cut].double(), b.engine.G[cut:].double()
        tn = torch.nn.utils.clip_grad_norm_([pw, pr], MAX_NORM)
        assert opt.param_groups[0]["lr"] == pytest.approx(table[k], rel=1e-12)
        opt.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.step()
        want = torch.cat([pw.detach(), pr.detach()])
        assert torch.allclose(a.engine.P.data.double(), want, rtol=0, atol=1e-7), float((a.engine.P.data - want).abs().max())
        for mine, theirs in state_of(a.engine, opt, pw, pr):
            assert torch.allclose(mine.double(), theirs, rtol=0, atol=1e-7)
            mine.copy_(theirs)
        a.engine.P.data.copy_(want)
        b.engine.P.data.copy_(want)
        assert float(sa.grad_norm[0]) == pytest.approx(float(tn), rel=1e-6)
        clipped += float(sa.grad_norm[1]) < 1.0
        assert sa.last_lr() == f32(table[k])
    assert clipped >= 1, "the clipping never acted: the comparison would not see it"
    name = "sgd_hp" if optimizer == "sgd" else "adam_hp"
    assert be.ran == ["grad_norm", name] * 3


def test_trainstep_warmup_cosine_adamw_clipping_equals_torch():
    make = lambda groups: torch.optim.AdamW(groups, lr=BASE_LR, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    state = lambda eng, opt, pw, pr: [(eng.adam_m, torch.cat([opt.state[pw]["exp_avg"], opt.state[pr]["exp_avg"]])),
                                      (eng.adam_v, torch.cat([opt.state[pw]["exp_avg_sq"], opt.state[pr]["exp_avg_sq"]]))]
    _three_steps_against_torch("adam", make, dict(weight_decay=WD, decay_mode="decoupled"), state)


def test_trainstep_warmup_cosine_sgd_l2_clipping_equals_torch():
    make = lambda groups: torch.optim.SGD(groups, lr=BASE_LR, momentum=0.9, nesterov=True, foreach=False)
    state = lambda eng, opt, pw, pr: [(eng.sgd_buf, torch.cat([opt.state[pw]["momentum_buffer"], opt.state[pr]["momentum_buffer"]]))]
    _three_steps_against_torch("sgd", make, dict(weight_decay=WD, decay_mode="l2", momentum=0.9, nesterov=True), state)


def test_engine_split_pair_equals_the_single_launch_bit_for_bit():
    """optim.Optimizer.split_ops as TrainStep drives it (main, counter - 1 into the tail counter, tail) against update_ops"""
    from video_classification_amd.optim import Optimizer
    a, b = _mini(seed=1), _mini(seed=1)
    gen = torch.Generator().manual_seed(9)
    table = torch.tensor(O.LR_TABLE)
    for mode, scope in (("decoupled", "weights"), ("l2", "all"), ("none", "weights")):
        kw = dict(weight_decay=O.WD, decay_mode=mode, decay_scope=scope)
        cut = a.engine.layers[1].w_off                            # the first layer's filters | the rest
        assert 0 < cut < a.engine.fc_b_off and cut % 4 == 0
        one = Optimizer(a.engine, lr_table=table, **kw).update_ops(grad_scale=0.5)
        main, tail, set_tail = Optimizer(b.engine, lr_table=table, **kw).split_ops(cut, grad_scale=0.5)
        for _ in range(2):
            g = torch.randn(a.engine.arena_numel, generator=gen)
            a.engine.G.copy_(g); b.engine.G.copy_(g)
            one(0)
            main(0)
            set_tail()
            tail(0)
            for x, y in ((a.engine.P.data, b.engine.P.data), (a.engine.adam_m, b.engine.adam_m), (a.engine.adam_v, b.engine.adam_v)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), mode
            assert int(a.engine.adam_step[0]) == int(b.engine.adam_step[0]) == int(b.engine.adam_step_tail[0])


def test_v2_trainer_refuses_decoupled_sgd():
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd.config import get_cfg
    from video_classification_amd.schedule import optim_kwargs
    cfg = get_cfg()
    cfg.MODEL.WEIGHT_DECAY = 0.01
    t = v2.Trainer.__new__(v2.Trainer)
    t.cfg, t.train_loader = cfg, [0] * 4
    with pytest.raises(ValueError, match="decoupled"):
        t._make_step(None, False, None)
    assert optim_kwargs(cfg, 4)["decay_mode"] == "decoupled"


# ------------------------------------------------------------------ the ABI of include/sfk_optim.h
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from video_classification_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfk_optim.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_OPTIM) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    assert lib.sfk_optim_abi_version() == _lib.OPTIM_ABI_VERSION == 1
    for n in ("adam_hp", "sgd_hp", "grad_norm", "grad_norm_parts"):
        assert callable(getattr(_lib.HipBackend, n))
    assert "optim_sched.hip" in open(os.path.join(ROOT, "video-classification_amd", "build.py")).read()


def test_struct_size_and_constants_match_the_header(lib, tmp_path):
    from video_classification_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_optim.h"\nint main(void){'
                   'printf("%zu %zu %zu %d %d %d %d\\n", sizeof(sfk_optim_hp), offsetof(sfk_optim_hp, clip_coef), '
                   'offsetof(sfk_optim_hp, weight_decay), SFK_DECAY_NONE, SFK_DECAY_L2, SFK_DECAY_DECOUPLED, '
                   'SFK_GRAD_NORM_MAX_PARTS);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # plain C, no HIP
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    H_ = _lib._OptimHp
    assert out[:3] == [ctypes.sizeof(H_), H_.clip_coef.offset, H_.weight_decay.offset]
    assert out[3:6] == [_lib.DECAY_MODES[k] for k in ("none", "l2", "decoupled")] and out[6] == _lib.GRAD_NORM_MAX_PARTS


def test_host_side_rejections_launch_nothing(lib):
    from video_classification_amd import _lib
    n = 8
    p, step, table = torch.zeros(n), torch.zeros(1, dtype=torch.int64), torch.ones(3)
    P, S, B = p.data_ptr(), step.data_ptr(), ctypes.byref

    def hp(**kw):
        d = _lib.new_optim_hp()
        d.lr_table, d.lr_len, d.decay_count, d.decay_mode = table.data_ptr(), 3, n, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    adam = lambda d, count=n: lib.sfk_adam_hp(P, P, P, P, count, B(d) if d is not None else None, 0.9, 0.999, 1e-8, 1.0, S, None, 0, None)
    sgd = lambda d, count=n: lib.sfk_sgd_hp(P, P, P, count, B(d) if d is not None else None, 0.9, 0.0, 0, 1.0, S, None, 0, None)
    bad = [hp(lr_table=None), hp(lr_len=0), hp(lr_len=-3), hp(decay_count=-1), hp(decay_count=n + 1), hp(decay_mode=3),
           hp(decay_mode=-1), hp(struct_size=0), hp(struct_size=ctypes.sizeof(_lib._OptimHp) - 8),
           hp(struct_size=ctypes.sizeof(_lib._OptimHp) + 8), None]
    for d in bad:
        assert adam(d) == -1 and sgd(d) == -1
    assert sgd(hp(decay_mode=2)) == -1                              # torch has no decoupled SGD
    assert adam(hp(), 0) == -1 and sgd(hp(), 0) == -1
    assert lib.sfk_adam_hp(None, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, S, None, 0, None) == -1
    assert lib.sfk_adam_hp(P, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, None, None, 0, None) == -1
    assert lib.sfk_adam_hp(P, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, S, P, 5, None) == -1
    assert lib.sfk_sgd_hp(P, P, None, n, B(hp()), 0.9, 0.0, 0, 1.0, S, None, 0, None) == -1      # momentum needs a buffer
    parts = torch.zeros(4, dtype=torch.float64)
    D = parts.data_ptr()
    assert lib.sfk_grad_norm(None, n, 1.0, 1.0, D, P, None) == -1 and lib.sfk_grad_norm(P, n, 1.0, 1.0, None, P, None) == -1
    assert lib.sfk_grad_norm(P, n, 1.0, 1.0, D, None, None) == -1 and lib.sfk_grad_norm(P, 0, 1.0, 1.0, D, P, None) == -1
    assert lib.sfk_grad_norm(P, n, 1.0, -1.0, D, P, None) == -1 and lib.sfk_grad_norm(P, n, 1.0, float("nan"), D, P, None) == -1
    assert lib.sfk_grad_norm_parts(0) == -1 and lib.sfk_grad_norm_parts(-5) == -1
    assert [lib.sfk_grad_norm_parts(c) for c in (1, 4096, 4097, 2048 * 4096, O.BIG, 1 << 40)] == [1, 1, 2, 2048, 2048, 2048]
    assert int(step[0]) == 0 and not p.any()


# ------------------------------------------------------------------ the trainers pass the keys through
def _v2_cfg(root):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT, cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.NUM_CLASS = str(root), 2, 4, 7
    cfg.MODEL.NAME, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DEPTH, cfg.NUM_CPU = "gesture-v2", 64, 18, 0
    cfg.MODEL.LR, cfg.MODEL.MAX_EPOCH = 1e-2, 2
    return cfg


def test_v2_trainer_follows_the_schedule_and_prints_rate_and_norm(tmp_path, capsys):
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd.schedule import lr_schedule
    cfg = _v2_cfg(tmp_path)
    cfg.MODEL.LR_SCHEDULE, cfg.MODEL.LR_WARMUP_STEPS, cfg.MODEL.LR_MIN = "cosine", 2, 1e-4
    cfg.MODEL.WEIGHT_DECAY, cfg.MODEL.WEIGHT_DECAY_MODE, cfg.MODEL.CLIP_GRAD_NORM = 0.01, "l2", 0.5
    tr = v2.SyntheticGesture(cfg, "train", num_videos=5, seed=1, h=48, w=64, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=3, clips_per_video=(1, 3), seed=2, h=48, w=64, min_box=8)
    be = Recorder()
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    assert t.steps_per_epoch() == 3 and t.step.hp and t.step.decay_mode == "l2" and t.step.clip_grad_norm == 0.5
    table = lr_schedule("cosine", 1e-2, 2, 3, warmup_steps=2, lr_min=1e-4)
    assert t.step.lr_table.tolist() == torch.tensor(table, dtype=F32).tolist()
    t.train_epoch()
    out = capsys.readouterr().out
    assert be.ran == ["grad_norm", "sgd_hp"] * 3 and int(t.model.engine.sgd_step[0]) == 3
    assert t.step.last_lr() == f32(table[2])
    assert f"lr: {f32(table[2]):.6g}, grad_norm: {float(t.step.grad_norm[0]):.4g}" in out
    cfg.MODEL.WEIGHT_DECAY_MODE = "decoupled"
    with pytest.raises(ValueError, match="decoupled"):
        v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=Recorder())


def test_default_trainer_prints_no_rate_line(tmp_path, capsys):
    from video_classification_amd import gesture_v2 as v2
    cfg = _v2_cfg(tmp_path)
    tr = v2.SyntheticGesture(cfg, "train", num_videos=2, seed=1, h=48, w=64, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=1, clips_per_video=(1, 1), seed=2, h=48, w=64, min_box=8)
    be = Recorder()
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    t.train_epoch()
    assert not t.step.hp and be.ran == ["sgd"] and "lr:" not in capsys.readouterr().out


def test_res2d_torch_backend_refuses_the_keys(tmp_path):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import Trainer
    for key, value in (("CLIP_GRAD_NORM", 1.0), ("WEIGHT_DECAY", 0.01), ("LR_SCHEDULE", "cosine")):
        cfg = get_cfg()
        cfg.CHALEARN.ROOT, cfg.MODEL.NAME, cfg.NUM_CPU = str(tmp_path), "res2d", 0
        cfg.MODEL[key] = value
        with pytest.raises(ValueError, match="RES2D_BACKEND"):
            Trainer(cfg, train_loader=[0, 0], test_loader=[0], device="cpu")
