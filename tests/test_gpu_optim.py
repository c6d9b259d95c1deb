"""include/sfk_optim.h on an MI355X, element by element against float64 (tests/optim_ref64.py): sfk_adam_hp and sfk_sgd_hp
over counts around the vector width, the block and the grid cap, every decay_count around its boundaries, steps before, at and
past the end of the rate table, slices that miss 16-byte alignment, both shadows, the clipping pointer and every decay mode;
sfk_grad_norm over the same counts with zero, inf and NaN inputs, bit-identical on a second run; the split pair against the
single launch; one launch captured into a graph and replayed along the table; the host-side rejections; TrainStep with the
schedule, decay and clipping against the fp32 oracle and against the float64 restatement.  tests/test_optim_cpu.py pins the
same tables without a GPU: honest float32 inside every bound, the mutations outside."""
import numpy as np
import pytest
import torch

import head_ref64 as H
import optim_ref64 as O
from emu_optim import EmuOptimBackend

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    return HipBackend()


def report(vs):
    print()
    for v in H.failures(vs):
        print(f"  {v}")
    print(f"  {len(vs)} verdicts, worst error/bound {H.worst_of(vs):.3g}")
    assert not H.failures(vs), H.failures(vs)[:5]


def _table(hip, count, kernel):
    vs = []
    for dc, s0, off, sh, clip, mi in O.hp_case_table(count):
        if kernel == "adam":
            vs += O.check_adam_hp(hip, DEV, count, dc, s0, off, sh, clip, O.MODES[mi])
        else:
            vs += O.check_sgd_hp(hip, DEV, count, dc, s0, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2))
    return vs


@pytest.mark.parametrize("count", O.COUNTS)
def test_adam_hp(hip, count):
    report(_table(hip, count, "adam"))


@pytest.mark.parametrize("count", O.COUNTS)
def test_sgd_hp(hip, count):
    report(_table(hip, count, "sgd"))


def test_every_option_crossed_at_one_count(hip):
    vs = []
    for off, sh, clip, mi in O.hp_cross_table():
        vs += O.check_adam_hp(hip, DEV, 1025, 5, 1, off, sh, clip, O.MODES[mi])
        vs += O.check_sgd_hp(hip, DEV, 1025, 5, 1, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2))
        vs += O.check_sgd_hp(hip, DEV, 1025, 5, 1, off, sh, clip, O.MODES[mi % 2], momentum=0.0)
    report(vs)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_update_just_above_the_grid_cap(hip, kernel):
    """cap x 1024 + 5 elements: the capped grid's second trip and the scalar tail; the decay boundary inside the second trip"""
    dc = O.GRID_CAP + 2
    if kernel == "adam":
        vs = O.check_adam_hp(hip, DEV, O.BIG, dc, len(O.LR_TABLE) + 5, 0, H.BF16, True, "decoupled")
        vs += O.check_adam_hp(hip, DEV, O.BIG, O.BIG, 0, 1, None, False, "l2")
    else:
        vs = O.check_sgd_hp(hip, DEV, O.BIG, dc, 1, 0, H.BF16, True, "l2", nesterov=True)
        vs += O.check_sgd_hp(hip, DEV, O.BIG, O.BIG, 0, 1, None, False, "l2")
    report(vs)


@pytest.mark.parametrize("count", O.COUNTS + [O.BIG])
def test_grad_norm(hip, count):
    vs = []
    for kind in ("randn", "zero", "inf", "nan"):
        for off in (0, 1):
            vs += O.check_grad_norm(hip, DEV, count, kind, off)
    vs += O.check_grad_norm(hip, DEV, count, "randn", 0, gscale=1.0, max_norm=1e6)       # the coefficient clamps at 1
    report(vs)


@pytest.mark.parametrize("count", [5, 4099, 3 * 2048 * 4096 // 2 + 7])
def test_grad_norm_is_bit_identical_on_a_second_run(hip, count):
    g = O.norm_inputs(count, DEV)
    st = torch.cuda.current_stream().cuda_stream
    rows = hip.grad_norm_parts(count)
    outs, parts = [], []
    for _ in range(2):
        p_, o_ = torch.zeros(rows, dtype=torch.float64, device=DEV), torch.zeros(2, device=DEV)
        hip.grad_norm(g, count, 0.5, 1.0, p_, o_)(st)
        torch.cuda.synchronize()
        outs.append(o_), parts.append(p_)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(parts[0].view(torch.int64), parts[1].view(torch.int64))
    assert float(outs[0][0]) > 0


def test_grad_norm_rows_depend_on_count_only(hip):
    emu = EmuOptimBackend()
    for count in (1, 3, 4096, 4097, 100_000, 2048 * 4096 - 1, 2048 * 4096, 2048 * 4096 + 1, O.BIG, 34_500_000, 1 << 33):
        assert hip.grad_norm_parts(count) == emu.grad_norm_parts(count) <= 2048, count


@pytest.mark.parametrize("count,dc", [(4099, 2048), (1025, 8)])
def test_split_pair_is_bit_equal_to_one_launch(hip, count, dc):
    vs = []
    cuts = sorted({c for c in (4, dc - 4, dc, dc + 4, count - count % 4 - 4) if 0 < c < count})
    assert all(c % 4 == 0 for c in cuts) and any(c < dc for c in cuts) and any(c > dc for c in cuts)
    for cut in cuts:
        for mode in O.MODES:
            vs += O.check_adam_hp_split(hip, DEV, count, cut, dc, 1, mode)
    report(vs)


def test_captured_launch_follows_the_table_on_replay(hip):
    """one sfk_adam_hp launch captured on a single stream and replayed three times against three eager launches, bit for bit,
    with three different rates: the rate is read from the table by the device's step counter, not baked into the graph"""
    count, dc = 4099, 2048
    gen = torch.Generator(device=DEV).manual_seed(77)
    p0, g0, m0, v0, _ = H.adam_inputs(count, 1, gen)
    table = torch.tensor(O.LR_TABLE, dtype=torch.float32, device=DEV)
    assert len(set(O.LR_TABLE[:3])) == 3
    coef = torch.tensor([O.COEF], device=DEV)
    (b1, b2), eps = H.ADAM_BETAS, H.ADAM_EPS

    def state():
        return [x.clone() for x in (p0, g0, m0, v0)] + [torch.zeros(1, dtype=torch.int64, device=DEV)]

    def launch(s):
        p, g, m, v, step = s
        return hip.adam_hp(p, g, m, v, count, table, b1, b2, eps, 0.5, step, None, weight_decay=O.WD, decay_mode="decoupled",
                           decay_count=dc, clip_coef=coef)
    eager = state()
    run = launch(eager)
    for _ in range(3):
        run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    replayed = state()
    run2 = launch(replayed)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run2(side.cuda_stream)                      # loads the code object outside the capture
    torch.cuda.synchronize()
    for x, x0 in zip(replayed, (p0, g0, m0, v0, torch.zeros(1, dtype=torch.int64, device=DEV))):
        x.copy_(x0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run2(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(replayed[4][0]) == int(eager[4][0]) == 3
    for a, b in zip(eager[:4], replayed[:4]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(eager[0], p0)


def test_host_side_rejections_launch_nothing(hip):
    from video_classification_amd._lib import SfkError
    n = 64
    st = torch.cuda.current_stream().cuda_stream
    p, g, m, v = (torch.full((n,), 0.5, device=DEV) for _ in range(4))
    step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    table = torch.ones(3, device=DEV)
    (b1, b2), eps = H.ADAM_BETAS, H.ADAM_EPS
    adam = lambda **kw: hip.adam_hp(p, g, m, v, n, table, b1, b2, eps, 1.0, step, None, **kw)
    sgd = lambda **kw: hip.sgd_hp(p, g, m, n, table, 0.9, 0.0, False, 1.0, step, None, **kw)
    bad = [dict(decay_count=-1), dict(decay_count=n + 1), dict(decay_mode=3), dict(decay_mode=-1)]
    for make in (adam, sgd):
        for kw in bad:
            with pytest.raises(SfkError, match="invalid"):
                make(**kw)(st)
    with pytest.raises(SfkError, match="invalid"):
        sgd(decay_mode="decoupled", decay_count=n)(st)
    torch.cuda.synchronize()
    assert int(step[0]) == 3 and all(bool((x == 0.5).all()) for x in (p, g, m, v))


# ------------------------------------------------------------------ TrainStep
def _mini(dtype=torch.float32):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=dtype, device=DEV)


def _clips(seed=5):
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(2, 4, 7, 64, 64, generator=g).permute(0, 2, 1, 3, 4)
    return [clips[:, 0:5], clips[:, 5:7]], torch.tensor([1, 4])


WARMUP, TOTAL, WD, MAX_NORM = 2, 6, 0.05, 1.0


def test_mini_model_scheduled_sgd_steps_match_oracle():
    """test_mini_v2_model_sgd_steps_match_oracle (tests/test_gpu_v2.py) with warm-up + cosine, L2 decay of the weights and
    clipping on both sides: torch's SGD(weight_decay) on the tensors of two or more dimensions, clip_grad_norm_, and
    SequentialLR(LinearLR, CosineAnnealingLR); the same tolerance policy.  (That policy judges the direction of each tensor's
    update, which is linear in the gradient under SGD; Adam's first steps are sign(g)-like and ill-conditioned where a gradient
    is near zero, so the Adam route is held to the float64 restatement below instead.)"""
    import warnings
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    from oracle import my_slowfast as o
    from test_engine_cpu import check_filter_copies, oracle_train_step_with_engine_mask, randomize
    from video_classification_amd.schedule import lr_schedule
    from video_classification_amd.train import TrainStep
    torch.manual_seed(1234)
    om = o.mini_slowfast(7, ref_style=True, depth=18, input_channels=(5, 2))
    randomize(om, 3)
    m = _mini()
    m.load_state_dict(om.state_dict(), strict=True)
    eng, lr, k = m.engine, 1e-2, 3
    x, labels = _clips()
    decayed = [p for p in om.parameters() if p.dim() > 1]
    rest = [p for p in om.parameters() if p.dim() <= 1]
    opt = torch.optim.SGD([dict(params=decayed, weight_decay=WD), dict(params=rest, weight_decay=0.0)], lr=lr, momentum=0.9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = SequentialLR(opt, [LinearLR(opt, start_factor=1.0 / WARMUP, end_factor=1.0, total_iters=WARMUP),
                                   CosineAnnealingLR(opt, T_max=TOTAL - WARMUP, eta_min=0.0)], milestones=[WARMUP])
    step = TrainStep(eng, lr=lr, optimizer="sgd", momentum=0.9, lr_table=lr_schedule("cosine", lr, 1, TOTAL, warmup_steps=WARMUP),
                     weight_decay=WD, decay_mode="l2", decay_scope="weights", clip_grad_norm=MAX_NORM)
    assert step.hp
    before = {kk: v.clone() for kk, v in om.state_dict().items()}
    xd, yd = [t.to(DEV) for t in x], labels.to(DEV)
    m.train()
    losses, norms = [], []
    for _ in range(k):
        _, loss_o = oracle_train_step_with_engine_mask(om, eng, x, labels)
        tn = float(torch.nn.utils.clip_grad_norm_(om.parameters(), MAX_NORM))
        opt.step()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.step()
        P_before = eng.P.data.clone()
        loss_m = float(step(xd[0], xd[1], yd))
        check_filter_copies(eng, P_before)
        losses.append((float(loss_o), loss_m))
        norms.append((tn, float(step.grad_norm[0]), float(step.grad_norm[1])))
    assert int(eng.sgd_step[0]) == k and eng.adam_step is None
    print("losses", losses, "norms (oracle, engine, coefficient)", norms)
    assert any(c < 1.0 for _, _, c in norms), "the clipping never acted"
    for i, (lo, lm) in enumerate(losses):
        tol = 1e-4 if i == 0 else (2e-2 if i == 1 else 0.2)
        assert abs(lo - lm) <= tol * max(abs(lo), 1e-3), losses
    for i, (tn, gn, _) in enumerate(norms):
        tol = 1e-4 if i == 0 else (2e-2 if i == 1 else 0.2)            # the norm is a function of the same gradients as the loss
        assert abs(tn - gn) <= tol * tn, norms
    sd_o, sd_m = om.state_dict(), m.state_dict()
    cos = []
    for kk in sd_o:
        a, b = sd_o[kk] - before[kk], sd_m[kk].cpu() - before[kk]
        if ".residual." in kk or ".res_unit." in kk:
            assert torch.equal(sd_o[kk], sd_m[kk].cpu()), kk
            continue
        if not a.is_floating_point() or a.abs().max() == 0:
            continue
        c = float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm() + 1e-30))
        r = float(b.double().norm() / a.double().norm())
        cos.append(c)
        lo_, hi_ = (0.9, 1.1) if a.numel() > 64 else (0.75, 1.33)
        assert lo_ < r < hi_, (kk, r)
    print("worst cosines", sorted(cos)[:3])
    assert min(cos) > 0.8 and float(np.median(cos)) > 0.985


@pytest.mark.parametrize("clip", [True, False], ids=["clipped-one-launch", "unclipped-split-pair"])
def test_trainstep_adamw_steps_match_the_float64_restatement(clip):
    """three AdamW steps of the depth-18 model, each held element by element to adam_hp_ref over the engine's own gradient
    arena: decay of [0, fc_b_off), the coefficient of sfk_grad_norm (clip) or the split pair beside the last kernel (no clip),
    and the rate of each step from the table"""
    from video_classification_amd.schedule import lr_schedule
    from video_classification_amd.train import TrainStep
    torch.manual_seed(7)
    m = _mini()
    eng = m.engine
    table = lr_schedule("cosine", 1e-3, 1, TOTAL, warmup_steps=WARMUP)
    step = TrainStep(eng, lr=1e-3, lr_table=table, weight_decay=WD, decay_mode="decoupled",
                     clip_grad_norm=MAX_NORM if clip else 0.0)
    x, labels = _clips(seed=11)
    xd, yd = [t.to(DEV) for t in x], labels.to(DEV)
    m.train()
    table32 = torch.tensor(table, dtype=torch.float32).tolist()
    (b1, b2), eps = (0.9, 0.999), 1e-8
    n, vs = eng.arena_numel, []
    for s in range(1, 4):
        p0 = eng.P.data.clone()
        m0 = eng.adam_m.clone() if eng.adam_m is not None else torch.zeros(n, device=DEV)
        v0 = eng.adam_v.clone() if eng.adam_v is not None else torch.zeros(n, device=DEV)
        step(xd[0], xd[1], yd)
        torch.cuda.synchronize()
        ops = next(iter(step._cache.values()))["ops"]
        assert ("grad_norm" in ops) == clip and not (clip and "adam_main" in ops)
        assert clip or ("adam_main" in ops) == bool(eng.two_streams and eng.options.split_adam)
        g = eng.G.clone()                                    # zero_grad runs before the backward: this step's gradients
        coef = None
        if clip:
            norm, c = O.grad_norm_ref(g, 1.0, MAX_NORM)
            vs.append(H.ElemOnly(H.compare(f"norm step {s}", step.grad_norm[0:1], norm.reshape(1), norm.reshape(1), 1, torch.float32, "map_f32")))
            coef = float(step.grad_norm[1])                  # the float32 the optimizer launch read
            vs.append(H.ElemOnly(H.compare(f"coef step {s}", step.grad_norm[1:2], c.reshape(1), c.reshape(1), 1, torch.float32, "map_f32")))
        r = O.adam_hp_ref(p0, g, m0, v0, s, table32, b1, b2, eps, 1.0, WD, "decoupled", eng.fc_b_off, coef)
        vs += [H.compare(f"m step {s}", eng.adam_m, r["m"], r["a_m"], 2, torch.float32, "map_f32"),
               H.compare(f"v step {s}", eng.adam_v, r["v"], r["a_v"], 2, torch.float32, "map_f32"),
               H.compare_p(f"p step {s}", eng.P.data, r),
               H.Exact(f"counter step {s}", int(eng.adam_step[0]) == s, "")]
        vs.append(H.Exact(f"rate step {s}", step.last_lr() == table32[s - 1], f"{step.last_lr()}"))
    report(vs)


@pytest.mark.parametrize("route", ["default", "table-decoupled", "clipped"])
def test_trainstep_issues_the_contract_launches(route, monkeypatch):
    """which optimizer launches two eager bf16 steps of the depth-18 model issue through TrainStep on HipBackend, derived
    from the contract, not recorded: without clipping the split pair -- [cut, n) with adam_step, then
    [0, cut) with adam_step_tail, cut = the plan's tail_cut, each with its slice-relative decay_count under the hp route;
    with clipping the norm, then ONE launch over [0, n) that reads the coefficient, and no pair"""
    from optim_trace import LaunchTrace
    from video_classification_amd.train import TrainStep
    torch.manual_seed(7)
    m = _mini(torch.bfloat16)
    eng = m.engine
    assert eng.two_streams and eng.options.split_adam
    tr = LaunchTrace(eng, monkeypatch.setattr)
    table = [1e-3, 5e-4, 2.5e-4]
    kw = {"default": {}, "table-decoupled": dict(lr_table=table, weight_decay=WD, decay_mode="decoupled"),
          "clipped": dict(clip_grad_norm=MAX_NORM)}[route]
    step = TrainStep(eng, lr=1e-3, **kw)
    x, labels = _clips(seed=11)
    xd, yd = [t.to(DEV) for t in x], labels.to(DEV)
    m.train()
    for _ in range(2):
        step(xd[0], xd[1], yd)
    torch.cuda.synchronize()
    (pl,) = eng._plans.values()
    (ent,) = step._cache.values()
    ops, n, dc, cut = ent["ops"], eng.arena_numel, eng.fc_b_off, pl.tail_cut[1]
    assert 0 < cut < dc < n
    built = tr.built
    ran = [built[i] for i in tr.ran]
    name = "adam" if route == "default" else "adam_hp"
    assert all(b["call"] == name for b in built if b["call"] != "grad_norm")

    def over(b, lo, hi, counter):
        """the launch b updates [lo, hi) of P, G, m and v with that counter"""
        want = [dict(arena=a, offset=lo, len=hi - lo) for a in ("P", "G", "adam_m", "adam_v")]
        return b["args"][:5] == want + [hi - lo] and b["args"][10] == dict(arena=counter, offset=0, len=1)

    if route == "clipped":
        assert "adam_main" not in ops and "adam_tail" not in ops and "grad_norm" in ops
        assert [b["call"] for b in ran] == ["grad_norm", "adam_hp"] * 2
        norm, upd = ran[0], ran[1]
        assert ran[2] is norm and ran[3] is upd
        assert norm["args"][0] == dict(arena="G", offset=0, len=n) and norm["args"][5] == dict(arena="grad_norm", offset=0, len=2)
        assert over(upd, 0, n, "adam_step") and upd["kwargs"]["clip_coef"] == dict(arena="grad_norm", offset=1, len=1)
        assert int(eng.adam_step[0]) == 2 and step.grad_norm is eng.grad_norm
        return
    assert "adam_main" in ops and "adam_tail" in ops and "grad_norm" not in ops
    assert [b["call"] for b in ran] == [name] * 4
    main, tail = ran[0], ran[1]
    assert ran[2] is main and ran[3] is tail
    assert over(main, cut, n, "adam_step") and over(tail, 0, cut, "adam_step_tail")
    if route == "table-decoupled":
        for b, count in ((main, min(max(dc - cut, 0), n - cut)), (tail, min(dc, cut))):
            assert b["kwargs"] == dict(weight_decay=WD, decay_mode="decoupled", decay_count=count, clip_coef="none")
            assert b["args"][5] == dict(table=torch.tensor(table, dtype=torch.float32).tolist())
        assert step.last_lr() == torch.tensor(table, dtype=torch.float32).tolist()[1]
    assert int(eng.adam_step[0]) == int(eng.adam_step_tail[0]) == 2
