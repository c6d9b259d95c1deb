"""include/sfk_ema.h on an MI355X.  sfk_ema_update bit for bit against tests/ref_ema.py computed on the CPU (counts around
the 16-byte unit and the 4096-element tile, arenas one element off alignment on either side, tables of 1 to 2048 elements,
every decay, warm-up flag and counter of ref_ema's lists), sentinels, sources and the counter; sfk_ema_swap as an exchange of
bits; one captured launch replayed against eager launches; the whole route on the mini SlowFast (eager, split and with one
optimizer launch behind a clipped norm) against the reference recursion over the same run's snapshots; evaluation
inside applied(), bit for bit; two mini epochs of each trainer.  tests/test_ema_cpu.py runs the same checks on the emulated backend and
shows that its mutants fail them.  The kernel has no grid cap and no loop over tiles, so there is no trip boundary to test
beyond the tile boundary at 4096."""
import pytest
import torch

import head_ref64 as H
import ref_ema as R

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
    print(f"  {len(vs)} verdicts")
    assert not H.failures(vs), H.failures(vs)[:5]


# ------------------------------------------------------------------ sfk_ema_update
@pytest.mark.parametrize("count", R.COUNTS)
def test_ema_update_bits(hip, count):
    cases = [c for c in R.update_cases() if c[0] == count]
    assert cases
    vs = []
    for case in cases:
        vs += R.check_ema_update(hip, DEV, *case)
    report(vs)


# ------------------------------------------------------------------ sfk_ema_swap
@pytest.mark.parametrize("count", R.COUNTS)
def test_ema_swap_exchanges_bits(hip, count):
    vs = []
    for case in [c for c in R.swap_cases() if c[0] == count]:
        vs += R.check_ema_swap(hip, DEV, *case)
    # the counter is not touched: HipBackend.ema_swap hands over none, so here the descriptor of an update goes to the swap
    import ctypes
    step = torch.tensor([41], dtype=torch.int64, device=DEV)
    pv, ev = R.swap_values(count, 3)
    p, e = pv.to(DEV), ev.to(DEV)
    d = hip._ema_desc(p, e, count, None, 0.9, True, step)
    hip._plain("sfk_ema_swap", ctypes.byref(d), keep=(d, p, e, step))(H._stream(DEV))
    torch.cuda.synchronize()
    vs.append(H.Exact("ema_swap counter", int(step[0]) == 41))
    vs.append(H.Exact("ema_swap with a counter", torch.equal(R._bits(p), R._bits(ev)) and torch.equal(R._bits(e), R._bits(pv))))
    report(vs)


# ------------------------------------------------------------------ one captured launch
def test_captured_update_advances_its_own_counter(hip):
    """an eager launch, then the launch captured and replayed three times with warm-up on, against three eager launches from
    the same state and against the recursion on the CPU: every replay reads the counter the one before it left"""
    count, decay = 4099, 0.999
    pv, ev = R.ema_values(count, 11)
    sv, dv = R.ema_values(257, 12)
    p, e, s, d = (t.to(DEV) for t in (pv, ev, sv, dv))
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    run = hip.ema_update(p, e, count, hip.ema_table([(s, d)]), decay, True, step)

    def restart():
        e.copy_(ev)
        d.copy_(dv)
        step.zero_()
    for _ in range(3):
        run(H._stream(DEV))
    torch.cuda.synchronize()
    eager = (e.cpu(), d.cpu(), int(step[0]))
    restart()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            run(stream.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(e.cpu(), ev) and int(step[0]) == 0          # capturing ran nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    want_e, want_d = ev, dv
    for t in (1, 2, 3):
        w = R.ema_weight(decay, True, t)
        want_e, want_d = R.ref_ema(want_e, pv, w), R.ref_ema(want_d, sv, w)
    assert len({R.ema_weight(decay, True, t) for t in (1, 2, 3)}) == 3
    assert eager[2] == 3 == int(step[0])
    assert torch.equal(R._bits(e), R._bits(eager[0])) and torch.equal(R._bits(d), R._bits(eager[1]))
    assert torch.equal(R._bits(e), R._bits(want_e)) and torch.equal(R._bits(d), R._bits(want_d))


# ------------------------------------------------------------------ the whole route
def _mini(dtype):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=dtype, device=DEV)


def _clips(dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    clips = torch.randn(2, 4, 7, 64, 64, generator=g).permute(0, 2, 1, 3, 4).to(DEV).to(dtype)
    return clips[:, 0:5].contiguous(), clips[:, 5:7].contiguous(), torch.tensor([1, 4], device=DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mode", ["eager", "clip"])
def test_train_step_keeps_the_reference_recursion(mode, dtype):
    """four steps with ema_decay 0.9 and warm-up on: ema_P and the averaged statistics equal the recursion over THIS run's
    snapshots of P / rm / rv (the filter gradients use atomics, so runs are never compared with each other).  'clip':
    clip_grad_norm, one optimizer launch, never split.  (The same under use_graph=True -- an eager step, the capture, two
    replays -- ended the capture in a host segmentation fault, bf16, on an MI355X; the cause was not found, the captured
    route was taken out of TrainStep and its case out of this test: DESIGN.md section 20.)"""
    from video_classification_amd.train import TrainStep
    m = _mini(dtype)
    eng = m.engine
    kw = dict(clip_grad_norm=1.0) if mode == "clip" else {}
    step = TrainStep(eng, lr=1e-2, ema_decay=0.9, ema_warmup=True, **kw)
    xs, xf, y = _clips(dtype)
    m.train()
    vs = R.check_route(eng, lambda: step(xs, xf, y), 4, 0.9, True)
    ops = next(iter(step._cache.values()))
    assert "ema" in ops["ops"]
    if mode == "clip":
        assert "adam_main" not in ops["ops"] and "grad_norm" in ops["ops"]
    print("ops", sorted(ops["ops"]))
    report(vs)


def test_captured_step_refuses_ema_before_it_builds_anything():
    from video_classification_amd.train import TrainStep
    m = _mini(torch.float32)
    with pytest.raises(ValueError, match="ema_decay.*eager"):
        TrainStep(m.engine, lr=1e-2, ema_decay=0.9, use_graph=True)
    assert m.engine.ema_P is None
    assert TrainStep(m.engine, lr=1e-2, ema_decay=0.0, use_graph=True).ema is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_applied_evaluates_the_averaged_model_and_restores_the_live_one(dtype):
    """inside applied() an eval forward gives the logits of a second engine loaded from ema.state_dict(), bit for bit
    (tests/test_gpu_model.py asserts torch.equal for two eval forwards of the same weights: the eval forward has no atomics);
    afterwards P / rm / rv hold the bits they held before and the live model's logits are its earlier ones, bit for bit"""
    from video_classification_amd.train import TrainStep
    m = _mini(dtype)
    eng = m.engine
    step = TrainStep(eng, lr=1e-2, ema_decay=0.9)
    xs, xf, y = _clips(dtype)
    m.train()
    for _ in range(3):
        step(xs, xf, y)
    before, avg = R.live_snapshot(eng), R.ema_snapshot(eng)
    assert not torch.equal(before[0], avg[0])
    m.eval()
    live_logits = m([xs, xf]).float().cpu()
    with step.ema.applied():
        assert torch.equal(R._bits(eng.P.data), R._bits(avg[0]))
        got = m([xs, xf]).float().cpu()
    after = R.live_snapshot(eng)
    assert all(torch.equal(R._bits(a), R._bits(b)) for a, b in zip(before, after))
    assert all(torch.equal(R._bits(a), R._bits(b)) for a, b in zip(avg, R.ema_snapshot(eng)))
    twin = _mini(dtype)
    twin.load_state_dict(step.ema.state_dict(), strict=True)
    twin.eval()
    want = twin([xs, xf]).float().cpu()
    assert torch.isfinite(want).all() and not torch.equal(want, live_logits)       # the averaged model is another model
    assert torch.equal(got, want)
    assert torch.equal(m([xs, xf]).float().cpu(), live_logits)


# ------------------------------------------------------------------ the trainers
@pytest.mark.parametrize("which,which_eval", [("v1", "ema"), ("v1", "both"), ("v2", "ema"), ("v1", "live")])
def test_trainer_epochs_with_ema_on(which, which_eval, tmp_path, capsys):
    """two mini epochs of each trainer with MODEL.EMA_DECAY set, asserting what the CPU trainer tests assert"""
    from test_ema_cpu import check_trainer_epochs, make_trainer
    t = make_trainer(which, tmp_path, device=DEV, DTYPE="bf16", EMA_DECAY=0.9, EMA_WARMUP=True, EMA_EVAL=which_eval)
    check_trainer_epochs(t, capsys, which_eval)
