"""MODEL.U8_STEM on an MI355X: the stem kernels reading uint8 frames through the table (include/sfk_u8stem.h) against
DevicePreprocess + the float entry points (forward and BatchNorm partial sums bit-identical, filter gradient to fp32
rounding) and against torch fp32; the models and the trainer with U8_STEM on and off; a captured TrainStep replayed on new
frames and crop offsets written into the same tensors."""
import pytest
import torch

from emu_stem2d import stem2d_ref
from emu_u8stem import materialize
from helpers import rel_err
from video_classification_amd._lib import FMap, HipBackend, StemSrc, stem_kp
from video_classification_amd.input_pipeline import DevicePreprocess, U8Clip, normalize_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def stem_weights(cout, c, kt, g):
    """random filters in the stem layout [co][((f*c + ci)*7 + kh)*8 + kw], zero at kw = 7 and in the tail"""
    w = torch.nn.functional.pad(torch.randn(cout, kt, c, 7, 7, generator=g) * 0.05, (0, 1)).reshape(cout, -1)
    return torch.nn.functional.pad(w, (0, stem_kp(c, kt) - w.shape[1])).reshape(-1)


def _crop(mode, n, pad, g):
    if mode is None:
        return None
    if mode == "zero":
        return torch.zeros(n, 2, dtype=torch.int32)
    if mode == "max":
        return torch.full((n, 2), 2 * pad, dtype=torch.int32)
    return torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32)


def run_both(kind, n, t, s, pitch, c0, c, dt, crop_mode, cout=64, seed=0, t_index=None, kt=1, check_torch=True):
    """kind '3d' (sfk_u8stem_conv_*) or '2d' (sfk_u8stem2d_*): the u8 stem against DevicePreprocess (f32) + float stem"""
    be = HipBackend()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(seed)
    pad = s // 10
    frames = torch.randint(0, 256, (n, t, s, s, pitch), generator=g, dtype=torch.uint8).to(DEV)
    crop = _crop(crop_mode, n, pad, g)
    crop = None if crop is None else crop.to(DEV)
    lut = normalize_lut().to(DEV)
    full = DevicePreprocess(DEV, be)(frames, crop, pad)                      # (n, t, pitch, s, s) f32
    xf = full.permute(0, 2, 1, 3, 4)[:, c0:c0 + c]                           # (n, c, t, s, s) strided view
    xu = U8Clip(frames, c0, c, crop, pad, lut)
    ti = None if t_index is None else torch.tensor(t_index, dtype=torch.int32, device=DEV)
    kt_ = t if kind == "2d" else kt
    sf, su = StemSrc(xf, ti, kt_), StemSrc(xu, ti, kt_)
    t_out = 1 if kind == "2d" else (t if ti is None else len(t_index))
    ho = (s - 1) // 2 + 1
    kp = stem_kp(c, kt_)
    w = stem_weights(cout, c, kt_, g).to(dt).to(DEV)
    y_f = FMap(torch.full((n * t_out * ho * ho * cout,), float("nan"), dtype=dt, device=DEV), n, t_out, ho, ho, cout)
    y_u = FMap(torch.full_like(y_f.buf, float("nan")), n, t_out, ho, ho, cout)
    fwd, wgrad = (be.stem2d_fwd, be.stem2d_wgrad) if kind == "2d" else (be.stem_conv_fwd, be.stem_conv_wgrad)
    ufwd, uwgrad = (be.u8stem2d_fwd, be.u8stem2d_wgrad) if kind == "2d" else (be.u8stem_conv_fwd, be.u8stem_conv_wgrad)
    mt = be.u8stem_tiles(su, y_u)
    assert mt == (be.stem2d_tiles if kind == "2d" else be.stem_conv_tiles)(sf, y_f)
    st_f, st_u = torch.zeros(mt * cout * 2, device=DEV), torch.full((mt * cout * 2,), float("nan"), device=DEV)
    fwd(sf, w, y_f, st_f)(stream)
    ufwd(su, w, y_u, st_u)(stream)
    dy = FMap((torch.randn(y_f.pixels * cout, generator=g) * 0.1).to(dt).to(DEV), n, t_out, ho, ho, cout)
    dw_f, dw_u = torch.zeros(cout * kp, device=DEV), torch.zeros(cout * kp, device=DEV)
    wgrad(sf, dy, dw_f)(stream)
    uwgrad(su, dy, dw_u)(stream)
    torch.cuda.synchronize()
    assert torch.equal(y_u.buf.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       y_f.buf.view(torch.int16 if dt == torch.bfloat16 else torch.int32))      # bit-identical
    assert torch.equal(st_u.view(torch.int32), st_f.view(torch.int32))
    assert torch.isfinite(dw_u).all() and rel_err(dw_u, dw_f) < 1e-5
    if check_torch:
        xr = materialize(U8Clip(frames.cpu(), c0, c, None if crop is None else crop.cpu(), pad, lut.cpu())).to(dt).float()
        assert torch.equal(xr, xf.cpu().to(dt).float())
        if kind == "2d":
            ref = stem2d_ref(xr, w.cpu().float(), cout)
        else:
            xs = xr if ti is None else xr.index_select(2, ti.cpu().long())
            wt = w.cpu().float().view(cout, kp)[:, :kt * c * 56].view(cout, kt, c, 7, 8)[..., :7].permute(0, 2, 1, 3, 4)
            ref = torch.nn.functional.conv3d(xs, wt, None, (1, 2, 2), (kt // 2, 3, 3))
        got = y_u.view5().float().cpu().permute(0, 4, 1, 2, 3)
        if dt == torch.float32:
            assert rel_err(got, ref) < 1e-4
        else:
            assert cosine(got, ref) > 0.9999 and rel_err(got, ref) < 1e-2
    return frames


CROPS = [None, "random", "zero", "max"]


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_u8_stem3d_cin5_kt1_gather(dt, crop):
    run_both("3d", 2, 8, 64, 21, 0, 5, dt, crop, t_index=[0, 2, 5, 7], kt=1, seed=1)


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_u8_stem3d_cin15_c0_5(dt, crop):
    """the reference SlowFast's fast stem: channels 5:20, kt 1, cout 8"""
    run_both("3d", 2, 4, 64, 21, 5, 15, dt, crop, cout=8, kt=1, seed=2)


@pytest.mark.parametrize("crop", ["random", "max"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_u8_stem3d_kt3_c0_5(dt, crop):
    """temporal taps and temporal padding with a channel offset (channels 5:10, kt 3)"""
    run_both("3d", 2, 4, 64, 21, 5, 5, dt, crop, cout=16, kt=3, seed=4)


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("pitch", [21, 5])
def test_u8_stem2d_t10_c5(pitch, dt, crop):
    run_both("2d", 2, 10, 64, pitch, 0, 5, dt, crop, seed=3)


@pytest.mark.parametrize("s", [128, 70])
@pytest.mark.parametrize("kind", ["3d", "2d"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_u8_stems_other_sizes(s, kind, dt):
    run_both(kind, 2, 3 if kind == "3d" else 10, s, 21, 0, 5, dt, "random", cout=32 if s == 70 else 64, seed=s)


def test_u8_stem2d_forward_res2d_yaml_size():
    """N 60, T 10, S 128 (res2d.yaml), bf16, random crops; cout 64: forward and statistics bit-identical"""
    run_both("2d", 60, 10, 128, 21, 0, 5, torch.bfloat16, "random", seed=5, check_torch=False)


def test_u8_stem_garbage_crop_is_memory_safe():
    """offsets far outside [0, 2*pad] mask everything they shift out of the frame, as DevicePreprocess's formula"""
    be = HipBackend()
    n, t, s = 3, 2, 64
    frames = torch.randint(0, 256, (n, t, s, s, 5), dtype=torch.uint8, device=DEV)
    crop = torch.tensor([[-(2 ** 31), 2 ** 31 - 1], [100000, -7], [40, 30]], dtype=torch.int32, device=DEV)
    lut = normalize_lut().to(DEV)
    x = U8Clip(frames, 0, 5, crop, 6, lut)
    ho = (s - 1) // 2 + 1
    w = stem_weights(64, 5, 1, torch.Generator().manual_seed(0)).to(DEV)
    y = FMap(torch.full((n * t * ho * ho * 64,), float("nan"), device=DEV), n, t, ho, ho, 64)
    be.u8stem_conv_fwd(StemSrc(x, None, 1), w, y, None)(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = y.view5().cpu()
    assert torch.equal(out[:2], torch.zeros_like(out[:2]))                 # clips 0 and 1 are all outside their frame
    ref = torch.nn.functional.conv3d(materialize(U8Clip(frames.cpu(), 0, 5, crop.cpu(), 6, lut.cpu())),
                                     w.cpu().view(64, -1)[:, :5 * 56].view(64, 1, 5, 7, 8)[..., :7].permute(0, 2, 1, 3, 4),
                                     None, (1, 2, 2), (0, 3, 3))
    assert rel_err(out.permute(0, 4, 1, 2, 3), ref) < 1e-4


# ------------------------------------------------------------------ models and the trainer
def _cfg(name, on, dtype="bf16"):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.BATCH_SIZE = 4
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.DTYPE = dtype
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.U8_STEM = on
    cfg.MODEL.LR = 1e-3
    cfg.NUM_CPU = 0
    cfg.DEBUG = True
    return cfg


def _trainer(name, on):
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = _cfg(name, on)
    tr = SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = SyntheticChalearn(cfg, "test", num_videos=3, clips_per_video=(1, 2), seed=2, as_uint8=True)
    torch.manual_seed(0)
    return Trainer(cfg, train_set=tr, test_set=te, device=DEV)


@pytest.mark.parametrize("name", ["res2d", "res3d", "slowfast"])
def test_trainer_u8_stem_on_and_off(name):
    ts = [_trainer(name, on) for on in (False, True)]
    # eval: identical scores
    ps = [t.run_eval()["ps"] for t in ts]
    assert (ps[0] == ps[1]).all()
    torch.manual_seed(3)
    batch = next(iter(ts[0].train_loader))
    xs = [t.mm.prepare_data(batch) for t in ts]
    assert torch.is_tensor(xs[0][0]) or torch.is_tensor(xs[0][0][0])
    assert isinstance(xs[1][0], U8Clip) or all(isinstance(v, U8Clip) for v in xs[1][0])
    # the first step through autograd: logits and loss bit-identical, gradients to rounding
    res = []
    for t, (x, y) in zip(ts, xs):
        t.model.train()
        logits = t.model(x)
        loss = torch.nn.functional.cross_entropy(logits.float(), y)
        loss.backward()
        torch.cuda.synchronize()
        res.append((logits.detach().clone(), loss.detach().clone(), t.model.engine.G.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # (the data gradients add split sums with fp32 atomics before they are rounded to bf16: an element that sits on a
    # rounding boundary can round either way, and that difference propagates down the network)
    assert rel_err(res[1][2], res[0][2]) < 2e-2 and cosine(res[1][2], res[0][2]) > 0.9999
    # three fused steps track each other
    losses = []
    for t, (x, y) in zip(ts, xs):
        one = []
        for _ in range(3):
            if isinstance(x, (torch.Tensor, U8Clip)):
                one.append(float(t.step(x, None, y)))
            else:
                one.append(float(t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)))
        losses.append(one)
    # Adam's first update is lr * sign(g) for every element, so gradient elements at rounding level (above) move by a full
    # lr either way and the runs drift apart as two float-path runs do; the losses stay on one track, measured against the
    # initial loss
    assert losses[0][0] == pytest.approx(losses[1][0], rel=1e-5), losses   # (the fused loss adds its batch with atomics)
    assert losses[0][-1] < losses[0][0] and losses[1][-1] < losses[1][0], losses
    for a, b in zip(*losses):
        assert abs(a - b) <= 5e-2 * losses[0][0], losses


def test_captured_train_step_follows_new_frames_and_crop():
    """TrainStep(use_graph=True) on a U8Clip; new frames and crop offsets written into the SAME tensors; the replay's loss
    equals an eager step of a copy of the model on those inputs"""
    from video_classification_amd.slowfast import resnet50_2d_engine
    from video_classification_amd.train import TrainStep
    g = torch.Generator().manual_seed(9)
    n, t, s = 4, 4, 64
    pad = s // 10
    frames = torch.randint(0, 256, (n, t, s, s, 21), generator=g, dtype=torch.uint8).to(DEV)
    crop = torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32).to(DEV)
    lut = normalize_lut().to(DEV)
    labels = torch.tensor([0, 3, 5, 1], device=DEV)
    m = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    step = TrainStep(m.engine, lr=1e-3, use_graph=True)
    x = U8Clip(frames, 0, 5, crop, pad, lut)
    step(x, None, labels)                      # eager
    step(x, None, labels)                      # captured + replayed
    old_loss = float(step(x, None, labels))    # replay
    frames.copy_(torch.randint(0, 256, frames.shape, generator=g, dtype=torch.uint8))
    crop.copy_(torch.tensor([[0, 2 * pad], [2 * pad, 0], [3, 7], [2 * pad, 2 * pad]], dtype=torch.int32))
    twin = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    twin.load_state_dict(m.state_dict(), strict=True)
    eager = TrainStep(twin.engine, lr=1e-3, use_graph=False)
    want = float(eager(U8Clip(frames.clone(), 0, 5, crop.clone(), pad, lut), None, labels))
    got = float(step(x, None, labels))         # replay of the captured graph
    assert step._cache and any(e["graph"] is not None for e in step._cache.values())
    assert got == pytest.approx(want, rel=1e-6, abs=1e-6) and got != old_loss
