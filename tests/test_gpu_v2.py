"""The v2 part-box trainer on an MI355X: sfk_roi_resize against CPU F.interpolate (both antialias settings, f32 and bf16,
boxes of every kind, crop shifts, HWC and planar sources, a captured graph following new boxes), sfk_sgd against
torch.optim.SGD, the mini v2 model's SGD steps against the oracle, the uint8 path against the float path, and the
gesture_v2 Trainer at the full v2 geometry in bf16."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from emu_v2 import roi_resize_ref
from test_engine_cpu import check_filter_copies, oracle_train_step_with_engine_mask, randomize
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import RoiResize, byte_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"

BOXES = {
    "down": [[10, 5, 250, 230], [0, 0, 320, 240]],
    "up": [[100, 100, 140, 150], [7, 9, 60, 40]],
    "nonsquare": [[3, 20, 300, 60], [50, 0, 70, 240]],
    "edge": [[0, 0, 100, 80], [220, 160, 320, 240]],
    "beyond": [[200, 150, 400, 300], [0, 10, 330, 250]],
    "15x15": [[0, 0, 15, 15], [305, 225, 320, 240]],
}
_frames_cache = {}


def frames(planar: bool):
    """(2, 2, 240, 320, 7) uint8 on the device: contiguous HWC, or a permuted view of planar (N, T, C, H, W) memory"""
    if planar not in _frames_cache:
        g = torch.Generator().manual_seed(4)
        x = torch.randint(0, 256, (2, 2, 7, 240, 320), generator=g, dtype=torch.uint8)
        _frames_cache[planar] = x.to(DEV).permute(0, 1, 3, 4, 2) if planar else x.permute(0, 1, 3, 4, 2).contiguous().to(DEV)
    return _frames_cache[planar]


def run_roi(src, box, s, aa, dtype, crop=None, pad=0, be=None):
    be = be or HipBackend()
    out = torch.full((src.shape[0], src.shape[1], src.shape[4], s, s), float("nan"), dtype=dtype, device=DEV)
    be.roi_resize(src, byte_lut().to(DEV), box, out, aa, crop, pad)(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("s", [64, 192])
@pytest.mark.parametrize("layout", ["hwc", "planar"])
@pytest.mark.parametrize("crop_mode", [None, "zero", "max"])
@pytest.mark.parametrize("case", list(BOXES))
@pytest.mark.parametrize("aa", [False, True], ids=["linear", "antialias"])
def test_roi_resize_matches_interpolate(aa, case, crop_mode, layout, s):
    src = frames(layout == "planar")
    box = torch.tensor(BOXES[case], dtype=torch.int32, device=DEV)
    pad = s // 10
    crop = None if crop_mode is None else torch.full((2, 2), 0 if crop_mode == "zero" else 2 * pad, dtype=torch.int32, device=DEV)
    got = run_roi(src, box, s, aa, torch.float32, crop, pad)
    want = roi_resize_ref(src.cpu(), byte_lut(), box.cpu(), s, s, aa, None if crop is None else crop.cpu(), pad)
    assert torch.isfinite(got).all()
    err = float((got.cpu() - want).abs().max())
    assert err <= 2e-6, err
    gb = run_roi(src, box, s, aa, torch.bfloat16, crop, pad)
    assert torch.equal(gb, got.to(torch.bfloat16))          # round to nearest even of the f32 result


def test_roi_resize_channel_offset_and_invalid_boxes_are_memory_safe():
    src = frames(False)
    be = HipBackend()
    out = torch.zeros(2, 2, 9, 64, 64, device=DEV)
    box = torch.tensor(BOXES["down"], dtype=torch.int32, device=DEV)
    be.roi_resize(src, byte_lut().to(DEV), box, out, True, c_off=2)(torch.cuda.current_stream().cuda_stream)
    want = roi_resize_ref(src.cpu(), byte_lut(), box.cpu(), 64, 64, True)
    assert float((out[:, :, 2:].cpu() - want).abs().max()) <= 2e-6 and out[:, :, :2].abs().sum() == 0
    bad = torch.tensor([[-50, 300, -3, 250], [400, -9, 1000, 2]], dtype=torch.int32, device=DEV)
    assert torch.isfinite(run_roi(src, bad, 64, True, torch.float32)).all()


def test_roi_resize_graph_follows_new_boxes():
    src = frames(False)
    be = HipBackend()
    box = torch.tensor(BOXES["down"], dtype=torch.int32, device=DEV)
    out = torch.empty(2, 2, 7, 192, 192, device=DEV)
    lut = byte_lut().to(DEV)
    run = be.roi_resize(src, lut, box, out, True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    for case in ("nonsquare", "15x15", "up"):
        box.copy_(torch.tensor(BOXES[case], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        want = roi_resize_ref(src.cpu(), byte_lut(), box.cpu(), 192, 192, True)
        assert float((out.cpu() - want).abs().max()) <= 2e-6, case


def within_ulp(a, b, scale):
    """|a - b| <= 1 ulp of `scale`: torch's GPU add(alpha=) fuses its multiply-add, sfk_sgd rounds the product first, so
    where the two terms cancel the results differ by one ulp of the TERMS, which can be several ulps of the small result"""
    return bool(((a - b).abs() <= torch.finfo(torch.float32).eps * scale.abs()).all())


@pytest.mark.parametrize("dampening,nesterov", [(0.0, False), (0.0, True), (0.1, False)])   # torch: Nesterov needs dampening 0
def test_sgd_matches_torch(dampening, nesterov):
    count, lr, mom, gs = 1_000_003, 0.05, 0.9, 0.5
    g0 = torch.Generator().manual_seed(9)
    p = torch.randn(count, generator=g0).to(DEV)
    buf = torch.zeros(count, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    shadow = torch.empty(count, dtype=torch.bfloat16, device=DEV)
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=mom, dampening=dampening, nesterov=nesterov, foreach=False)
    be = HipBackend()
    for k in range(5):
        g = torch.randn(count, generator=g0).to(DEV)
        p0, b0 = p.clone(), buf.clone()
        be.sgd(p, g, buf, count, lr, mom, dampening, nesterov, gs, step, shadow)(torch.cuda.current_stream().cuda_stream)
        tp.grad = g * gs
        opt.step()
        torch.cuda.synchronize()
        assert int(step[0]) == k + 1
        tb = opt.state[tp]["momentum_buffer"]
        bterms = (g * gs).abs() if k == 0 else (mom * b0).abs() + ((1 - dampening) * g * gs).abs()
        d = (g * gs).abs() + mom * tb.abs() if nesterov else tb.abs()
        assert within_ulp(buf, tb, bterms) and within_ulp(p, tp.detach(), p0.abs() + lr * d), k
        assert torch.equal(shadow, p.to(torch.bfloat16))
        with torch.no_grad():                            # per step: the next step starts from the same state
            tp.copy_(p)
            opt.state[tp]["momentum_buffer"].copy_(buf)


def _cfg(dtype="fp32", t=4, size=64, bs=2, depth=18, root="/nonexistent"):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = t
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "gesture-v2"
    cfg.MODEL.INPUT_SIZE = size
    cfg.MODEL.DEPTH = depth
    cfg.MODEL.DTYPE = dtype
    cfg.NUM_CPU = 0
    return cfg


def test_mini_v2_model_sgd_steps_match_oracle():
    from oracle import my_slowfast as o
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    from video_classification_amd.train import TrainStep
    torch.manual_seed(1234)
    om = o.mini_slowfast(7, ref_style=True, depth=18, input_channels=(5, 2))
    randomize(om, 3)
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    m = SlowFast(spec, dtype=torch.float32, device=DEV)
    m.load_state_dict(om.state_dict(), strict=True)
    eng, lr, k = m.engine, 1e-2, 3
    g = torch.Generator().manual_seed(5)
    clips = torch.randn(2, 4, 7, 64, 64, generator=g).permute(0, 2, 1, 3, 4)
    x = [clips[:, 0:5], clips[:, 5:7]]
    labels = torch.tensor([1, 4])
    opt = torch.optim.SGD(om.parameters(), lr=lr, momentum=0.9)
    step = TrainStep(eng, lr=lr, optimizer="sgd", momentum=0.9)
    before = {kk: v.clone() for kk, v in om.state_dict().items()}
    xd, yd = [t.to(DEV) for t in x], labels.to(DEV)
    m.train()
    losses = []
    for _ in range(k):
        _, loss_o = oracle_train_step_with_engine_mask(om, eng, x, labels)
        opt.step()
        P_before = eng.P.data.clone()
        loss_m = float(step(xd[0], xd[1], yd))
        check_filter_copies(eng, P_before)
        losses.append((float(loss_o), loss_m))
    assert int(eng.sgd_step[0]) == k and eng.adam_step is None
    for i, (lo, lm) in enumerate(losses):
        tol = 1e-4 if i == 0 else (2e-2 if i == 1 else 0.2)
        assert abs(lo - lm) <= tol * max(abs(lo), 1e-3), losses
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
    print("losses", losses, "worst cosines", sorted(cos)[:3])
    assert min(cos) > 0.8 and float(np.median(cos)) > 0.985


def _preprocess_host(frames_u8, box, s):
    """the reference's _features_from_indices + _preprocess (new_feature_test.py:590-661), restated: crop, /255, Resize"""
    out = {"rgb": [], "uv": [], "flow": []}
    for i in range(frames_u8.shape[0]):
        x1, y1, x2, y2 = box[i].tolist()
        X = frames_u8[i, :, y1:y2, x1:x2].permute(0, 3, 1, 2).to(torch.float32).div(255)
        X = F.interpolate(X, (s, s), mode="bilinear", align_corners=False, antialias=True)
        rgb, uv, flow = torch.tensor_split(X, [3, 5], dim=1)
        out["rgb"].append(rgb), out["uv"].append(uv), out["flow"].append(flow)
    return {k: torch.stack(v) for k, v in out.items()}


def test_uint8_path_matches_float_path():
    from video_classification_amd import gesture_v2 as v2
    g = torch.Generator().manual_seed(8)
    fr = torch.randint(0, 256, (2, 4, 120, 160, 7), generator=g, dtype=torch.uint8)
    box = torch.tensor([[10, 4, 110, 117], [37, 0, 160, 90]], dtype=torch.int32)
    label = torch.tensor([2, 6])
    ub = {"frames_u8": fr, "box": box, "label": label}
    fb = dict(_preprocess_host(fr, box, 64), label=label)
    mm = v2.ModelManager(_cfg("fp32"), DEV)
    m = mm.init_model()
    m.eval()
    with torch.no_grad():
        xu, _ = mm.prepare_data(ub)
        lu = m(xu).float().cpu()
        xf, _ = mm.prepare_data(fb)
        lf = m(xf).float().cpu()
    err = float((lu - lf).abs().max())
    print("uint8 vs float logits", err)
    assert err <= 1e-4 * max(1.0, float(lf.abs().max()))
    # bf16: the bf16 resize output and the f32 one give bit-identical logits (the stems round f32 to bf16 on staging)
    mb = v2.ModelManager(_cfg("bf16"), DEV)
    assert mb.roi_resize().out_dtype == torch.bfloat16
    model = mb.init_model()
    model.eval()
    with torch.no_grad():
        xb, _ = mb.prepare_data(ub)
        assert xb[0].dtype == torch.bfloat16
        lb = model(xb).float().cpu()
        x32 = RoiResize(64, DEV, out_dtype=torch.float32)(fr, box).permute(0, 2, 1, 3, 4)
        l32 = model([x32[:, 0:5], x32[:, 5:7]]).float().cpu()
    assert torch.equal(lb, l32)


def test_v2_trainer_full_geometry_bf16(tmp_path):
    from video_classification_amd import gesture_v2 as v2
    cfg = _cfg("bf16", t=20, size=192, bs=10, depth=50, root=tmp_path)
    cfg.CHALEARN.NUM_CLASS = 249
    cfg.MODEL.LR = 1e-3
    tr = v2.SyntheticGesture(cfg, "train", num_videos=13, seed=1)           # 10 + a short batch of 3
    te = v2.SyntheticGesture(cfg, "test", num_videos=3, clips_per_video=(1, 2), seed=2)
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    loss, _ = t.train_epoch()                     # the mean of the epoch's step losses: finite only if each one is
    assert t.step.steps == math.ceil(13 / 10) == 2 and int(t.model.engine.sgd_step[0]) == 2
    assert math.isfinite(loss)
    ev = t.run_eval()
    assert set(ev) == {"ps", "t", "acc", "sv"} and ev["ps"].shape == (sum(te.nclips), 249)
    assert np.isfinite(ev["ps"]).all() and np.allclose(ev["ps"].sum(1), 1, atol=1e-4)
    t.save_ckpt(epoch=0, acc=float(ev["acc"]))
    sd = t.model.state_dict()
    m2 = v2.ModelManager(cfg, DEV).init_model()
    m2.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    t2 = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)              # load_ckpt, strict=True
    assert torch.equal(t2.model.engine.P.data, t.model.engine.P.data)
