"""include/sfk_mix.h on an MI355X.  sfk_clip_mix bit for bit against tests/ref_mix.py computed on the CPU (frames that take
the scalar rows and tails, 17x19, and the 16-byte path, 32x32; three layouts; 1, 2, 5 and 6 clips; f32 and bf16; every pair
spec of ref_mix.pair_specs), with everything outside the mixed channels, identity pairs and self clips unchanged and a second
run giving the same bits; sfk_softmax_ce_mix element by element against the float64 restatement; the whole route: the mini
SlowFast against the oracle on the torch-mixed clip, a captured step following new rows, one mini epoch of each trainer.
tests/test_mix_cpu.py runs the same checks on the emulated backend and shows that its mutants fail them.  No case hands the
kernel an out-of-range partner: that guard is stated in the header and exercised on the emulated backend only."""
import math

import pytest
import torch

import head_ref64 as H
import ref_mix as R

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


# ------------------------------------------------------------------ sfk_clip_mix
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", R.MIX_N)
@pytest.mark.parametrize("layout", list(R.MIX_LAYOUTS))
@pytest.mark.parametrize("h,w", R.MIX_SIZES)
def test_clip_mix_bits(hip, h, w, layout, n, dtype):
    report(R.check_clip_mix(hip, DEV, h, w, layout, n, dtype))


@pytest.mark.parametrize("h,w", R.MIX_SIZES)
def test_bf16_equals_f32_kernel_rounded(hip, h, w):
    st = torch.cuda.current_stream().cuda_stream
    xb = R.mix_input(6, 2, 7, h, w, torch.bfloat16)
    for rows in R.mix_row_sets(6, h, w):
        vb, _ = R.on_device(xb, DEV, 0, torch.bfloat16)
        vf, _ = R.on_device(xb.float(), DEV, 0, torch.float32)
        hip.clip_mix(vb, rows.to(DEV))(st)
        hip.clip_mix(vf, rows.to(DEV))(st)
        torch.cuda.synchronize()
        assert torch.equal(vb, vf.to(torch.bfloat16))


def test_captured_launch_follows_new_rows(hip):
    h, w, n = 32, 32, 6
    sets = R.mix_row_sets(n, h, w)
    x = R.mix_input(n, 2, 7, h, w, torch.float32)
    view, _ = R.on_device(x, DEV)
    table = sets[0].to(DEV)
    hip.clip_mix(view, table)(torch.cuda.current_stream().cuda_stream)      # eager once: the code object is loaded
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            hip.clip_mix(view, table)(s.cuda_stream)
    got = []
    for rows in (sets[0], sets[3], sets[1]):
        view.copy_(x)
        table.copy_(rows.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(view.cpu(), R.ref_mix(x, rows))
        got.append(view.cpu())
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


# ------------------------------------------------------------------ sfk_softmax_ce_mix
@pytest.mark.parametrize("case", R.CE_MIX_CASES, ids=lambda c: f"k{c[0]}-n{c[1]}-eps{c[2]}-{c[3]}")
def test_softmax_ce_mix(hip, case):
    report(R.check_ce_mix(hip, DEV, case))


def test_softmax_ce_mix_judges_the_heavier_label_and_counts_the_first_maximum(hip):
    report(R.check_ce_mix_correct(hip, DEV))


# ------------------------------------------------------------------ the whole route
ROUTE_ROWS = [[3, 0.35, 0, 0, 0, 0, 0.35, 0], [2, 1.0, 8, 20, 40, 52, 0.75, 0],
              [1, 1.0, 8, 20, 40, 52, 0.75, 0], [0, 0.35, 0, 0, 0, 0, 0.35, 0]]      # one mixup pair, one CutMix pair (32 x 32 of 64 x 64)


def test_mini_model_mixed_smoothed_sgd_steps_match_oracle(hip):
    """three fp32 steps of the depth-18 (5, 2) SlowFast on four mixed clips with eps = 0.1; the oracle runs on the torch-mixed
    clip with the smoothed probability matrix as its target (F.cross_entropy takes probabilities); the loss tolerances of
    steps 1, 2, 3 are test_mini_model_scheduled_sgd_steps_match_oracle's"""
    from oracle import my_slowfast as o
    from test_engine_cpu import oracle_train_step_with_engine_mask, randomize
    from test_gpu_optim import _mini
    from video_classification_amd.input_pipeline import ClipMix
    from video_classification_amd.train import TrainStep
    torch.manual_seed(1234)
    om = o.mini_slowfast(7, ref_style=True, depth=18, input_channels=(5, 2))
    randomize(om, 3)
    m = _mini()
    m.load_state_dict(om.state_dict(), strict=True)
    eng, lr, eps, k = m.engine, 1e-2, 0.1, 7
    g = torch.Generator().manual_seed(5)
    clip = torch.randn(4, 4, 7, 64, 64, generator=g)                       # (N, T, C, S, S), as prepare_data holds it
    labels = torch.tensor([1, 4, 2, 6])
    rows = torch.tensor(ROUTE_ROWS, dtype=torch.float32)
    w, p = rows[:, 6:7], rows[:, 0].long()
    onehot = torch.nn.functional.one_hot(labels, k).float()
    target = (1 - eps) * (w * onehot + (1 - w) * onehot[p]) + eps / k
    mixed = R.ref_mix(clip, rows).permute(0, 2, 1, 3, 4)
    xo = [mixed[:, 0:5], mixed[:, 5:7]]
    opt = torch.optim.SGD(om.parameters(), lr=lr, momentum=0.9)
    step = TrainStep(eng, lr=lr, optimizer="sgd", momentum=0.9, label_smoothing=eps)
    cm = ClipMix(DEV, hip, batch_size=4)
    yd, dev_clip = labels.to(DEV), torch.empty(clip.shape, device=DEV)
    m.train()
    losses = []
    for _ in range(3):
        _, loss_o = oracle_train_step_with_engine_mask(om, eng, xo, target)
        opt.step()
        table = cm.load(rows, 64, 64)
        dev_clip.copy_(clip)
        xd = cm(dev_clip, table).permute(0, 2, 1, 3, 4)
        assert torch.equal(xd.cpu(), mixed)
        losses.append((float(loss_o), float(step(xd[:, 0:5], xd[:, 5:7], yd, mix=table))))
    print("losses (oracle, engine)", losses)
    for i, (lo, lm) in enumerate(losses):
        tol = 1e-4 if i == 0 else (2e-2 if i == 1 else 0.2)
        assert abs(lo - lm) <= tol * max(abs(lo), 1e-3), losses


def test_captured_train_step_follows_new_rows(hip):
    """TrainStep(use_graph=True, label_smoothing=0.1) on the res2d engine with mix= the ClipMix table; new rows written into the
    SAME table and the next clip mixed by them; the replay's loss equals an eager step of a copy of the model on those rows"""
    from video_classification_amd.input_pipeline import ClipMix
    from video_classification_amd.slowfast import resnet50_2d_engine
    from video_classification_amd.train import TrainStep
    g = torch.Generator().manual_seed(9)
    n, t, s = 4, 4, 64
    src = torch.randn(n, t, 5, s, s, generator=g).to(torch.bfloat16)
    labels = torch.tensor([0, 3, 5, 1], device=DEV)
    rows_a = torch.tensor(ROUTE_ROWS, dtype=torch.float32)
    rows_b = torch.tensor([[1, 0.8, 0, 0, 0, 0, 0.8, 0], [0, 0.8, 0, 0, 0, 0, 0.8, 0],
                           [3, 1.0, 0, 0, 64, 32, 0.5, 0], [2, 1.0, 0, 0, 64, 32, 0.5, 0]], dtype=torch.float32)
    m = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    step = TrainStep(m.engine, lr=1e-3, use_graph=True, label_smoothing=0.1)
    cm = ClipMix(DEV, hip, batch_size=n)
    x = torch.empty(n, t, 5, s, s, dtype=torch.bfloat16, device=DEV)        # the clip's address is part of the captured step

    def mixed_step(st, rows, clip, mixer):
        table = mixer.load(rows, s, s)
        clip.copy_(src)
        mixer(clip, table)
        return float(st(clip, None, labels, mix=table))
    mixed_step(step, rows_a, x, cm)                  # eager
    mixed_step(step, rows_a, x, cm)                  # captured + replayed
    old_loss = mixed_step(step, rows_a, x, cm)       # replay
    twin = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    twin.load_state_dict(m.state_dict(), strict=True)
    eager = TrainStep(twin.engine, lr=1e-3, use_graph=False, label_smoothing=0.1)
    want = mixed_step(eager, rows_b, torch.empty_like(x), ClipMix(DEV, hip, batch_size=n))
    got = mixed_step(step, rows_b, x, cm)            # replay of the captured graph on the new rows
    assert step._cache and any(e["graph"] is not None for e in step._cache.values()) and len(step._cache) == 1
    assert got == pytest.approx(want, rel=1e-6, abs=1e-6) and got != old_loss


@pytest.mark.parametrize("which", ["v1", "v2"])
def test_trainer_epoch_with_the_keys_on(which, tmp_path):
    """one mini epoch of each trainer with mixing and smoothing on: what prepare_data hands the model is ref_mix of what it
    hands over without the entry, bit for bit, and the epoch's loss is finite"""
    from test_mix_cpu import MIX_ON, _cat, _cfg, _spy, _v1_sets
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd import train as v1
    cfg = _cfg("gesture-v2" if which == "v2" else "slowfast-LHand", **MIX_ON)
    cfg.MODEL.DTYPE = "bf16"
    if which == "v2":
        cfg.CHALEARN.ROOT = str(tmp_path)
        tr = v2.SyntheticGesture(cfg, "train", num_videos=3, seed=1, h=48, w=64, min_box=8)
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
        t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    else:
        tr, te = _v1_sets(cfg)
        t = v1.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    seen = []
    _spy(t, seen)
    loss, _ = t.train_epoch()
    assert math.isfinite(loss) and len(seen) == 2
    for rows, before, x in seen:
        want = R.ref_mix(_cat(before).permute(0, 2, 1, 3, 4).cpu(), rows.cpu()).permute(0, 2, 1, 3, 4)
        assert torch.equal(_cat(x).cpu(), want)
    assert not torch.equal(_cat(seen[0][2]), _cat(seen[0][1]))
