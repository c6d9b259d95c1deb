"""The res2d network on an MI355X: the frames-as-channels stem kernels (include/sfk_stem2d.h) against torch-CPU fp32, the
whole model against res2d.py's torch.nn ResNet2d, and the trainer with MODEL.RES2D_BACKEND = 'engine'."""
import numpy as np
import pytest
import torch

from emu_stem2d import stem2d_ref
from helpers import rel_err, rel_l2
from video_classification_amd import arch
from video_classification_amd._lib import FMap, HipBackend, StemSrc, stem_kp
from video_classification_amd.res2d import ResNet2d, resnet50_2d

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def stem_layout(w4, t):
    """(cout, t*5, 7, 7) -> [co][((t*5 + c)*7 + kh)*8 + kw] (zero padded)"""
    co = w4.shape[0]
    w = torch.nn.functional.pad(w4.reshape(co, t * 5, 7, 7), (0, 1)).reshape(co, -1)
    return torch.nn.functional.pad(w, (0, stem_kp(5, t) - w.shape[1])).reshape(-1)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("cout", [64, 32])
@pytest.mark.parametrize("t", [1, 2, 10])
@pytest.mark.parametrize("s", [64, 130])
@pytest.mark.parametrize("dt,src_dt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                       (torch.bfloat16, torch.float32)], ids=["f32", "bf16", "bf16-f32src"])
def test_stem2d_kernels_match_torch_cpu(t, s, dt, src_dt, cout, n=3):
    be = HipBackend()
    g = torch.Generator().manual_seed(t * 1000 + s)
    clip = torch.randn(n, t, 21, s, s, generator=g).to(src_dt)          # the loader's memory; the stem reads [:, :, :5]
    x5 = clip.to(DEV)[:, :, :5].permute(0, 2, 1, 3, 4)                  # (N, 5, T, S, S) strided view, no copy
    w4 = torch.randn(cout, t * 5, 7, 7, generator=g) * 0.05
    w = stem_layout(w4, t).to(dt).to(DEV)
    ho = wo = (s - 1) // 2 + 1
    y = FMap(torch.full((n * ho * wo * cout,), float("nan"), dtype=dt, device=DEV), n, 1, ho, wo, cout)
    src = StemSrc(x5, None, t)
    mt = be.stem2d_tiles(src, y)
    assert mt == n * ((ho + 15) // 16) ** 2
    stats = torch.zeros(mt * cout * 2, device=DEV)
    be.stem2d_fwd(src, w, y, stats)(torch.cuda.current_stream().cuda_stream)
    xr = clip[:, :, :5].permute(0, 2, 1, 3, 4).to(dt).float()           # the clip as the kernel stages it
    ref = stem2d_ref(xr, w.cpu().float(), cout)                           # (N, cout, 1, ho, wo)
    got = y.view5().float().cpu().permute(0, 4, 1, 2, 3)
    # per-tile partial sums, tile = (n * tiles_h + th) * tiles_w + tw: the layout sfk_bn_finalize consumes
    tpe = (ho + 15) // 16
    r = torch.nn.functional.pad(ref[:, :, 0].double(), (0, 16 * tpe - wo, 0, 16 * tpe - ho))
    r = r.view(n, cout, tpe, 16, tpe, 16)
    want_tiles = torch.stack([r.sum((3, 5)), (r * r).sum((3, 5))], -1).permute(0, 2, 3, 1, 4).reshape(mt, cout, 2)
    st_tiles = stats.view(mt, cout, 2).cpu().double()
    st = st_tiles.sum(0)
    want_s1, want_s2 = want_tiles[..., 0].sum(0), want_tiles[..., 1].sum(0)
    assert rel_err(st_tiles, want_tiles) < (1e-4 if dt == torch.float32 else 1e-3)
    if dt == torch.float32:
        assert rel_err(got, ref) < 1e-4
        assert rel_err(st[:, 0], want_s1) < 1e-4 and rel_err(st[:, 1], want_s2) < 1e-4
    else:
        assert cosine(got, ref) > 0.9999 and rel_err(got, ref) < 1e-2
        assert rel_err(st[:, 0], want_s1) < 1e-3 and rel_err(st[:, 1], want_s2) < 1e-3
    # filter gradient from a random dY (written over a NaN-filled dw: the kernel overwrites all of it)
    dy = FMap((torch.randn(n * ho * wo * cout, generator=g) * 0.1).to(dt).to(DEV), n, 1, ho, wo, cout)
    dw = torch.full((cout * stem_kp(5, t),), float("nan"), device=DEV)
    be.stem2d_wgrad(src, dy, dw)(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with torch.enable_grad():
        wt = torch.zeros(cout, 5, t, 7, 7, requires_grad=True)
        out = torch.nn.functional.conv3d(xr, wt, None, (1, 2, 2), (0, 3, 3))
        out.backward(dy.view5().float().cpu().permute(0, 4, 1, 2, 3))
    want = stem_layout(wt.grad.permute(0, 2, 1, 3, 4).reshape(cout, t * 5, 7, 7), t)
    got_dw = dw.cpu()
    assert torch.isfinite(got_dw).all()
    assert rel_err(got_dw, want) < (1e-4 if dt == torch.float32 else 1e-3)
    rows = got_dw.view(cout, -1)
    assert not rows[:, t * 5 * 56:].any() and not rows[:, :t * 5 * 56].view(cout, -1, 8)[..., 7].any()   # padding stays 0


def test_stem2d_kernels_f32_map_from_a_bf16_clip():
    """the pairing the cases above leave out (the <float, bf16_t> kernels), at the smallest shape with more than one tile per
    axis and a partial last tile: 36 x 36 frames -> 18 x 18 output, 15 planes = three full chunks and one of three planes"""
    test_stem2d_kernels_match_torch_cpu(3, 36, torch.float32, torch.bfloat16, 64, n=2)


# ------------------------------------------------------------------ whole model
def _randomize(model, seed):
    """random running statistics; block-final BatchNorm weights 0.2.  (With torchvision's init -- every gamma 1 -- the
    untrained ResNet-50's residual sums grow block after block and the N = 2 gradient at the stem is chaotic: bf16 against
    fp32 cosines fall to ~0.1 there at depth 50 while the depth-18 wiring gives 0.95.  Scaled block outputs, as in a
    trained network, keep the comparison about the kernels.)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith(("bn3.weight", "downsample.1.weight")):
                v.fill_(0.2)
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)


def _pair(crop, dtype, seed=7):
    from video_classification_amd.slowfast import resnet50_2d_engine
    torch.manual_seed(seed)
    om = resnet50_2d(50, 1000)
    _randomize(om, seed)
    m = resnet50_2d_engine(1000, 10, crop, dtype=dtype, device=DEV, backend=HipBackend())
    m.load_state_dict(om.state_dict(), strict=True)
    return om, m


@pytest.mark.parametrize("crop", [128, 192])
def test_model_forward_and_step_against_resnet2d_fp32(crop):
    om, m = _pair(crop, torch.float32)
    clips = torch.randn(2, 10, 21, crop, crop, generator=torch.Generator().manual_seed(crop))
    x = clips[:, :, :5].reshape(2, 50, crop, crop)
    om.eval(); m.eval()
    with torch.no_grad():
        want = om(x)
        got = m(clips.to(DEV)[:, :, :5]).float().cpu()
    err = rel_err(got, want)
    print(f"res2d {crop} fp32: eval logits rel err {err:.2e}")
    assert err < 1e-3
    om.train(); m.train()
    labels = torch.tensor([3, 17])
    loss_o = torch.nn.functional.cross_entropy(om(x), labels)
    loss_o.backward()
    y = m(clips.to(DEV)[:, :, :5])
    loss_m = torch.nn.functional.cross_entropy(y, labels.to(DEV))
    loss_m.backward()
    assert abs(float(loss_m.detach()) - float(loss_o.detach())) < 1e-3 * float(loss_o.detach())
    gsd = _engine_grads(m.engine)
    cos = {k: cosine(gsd[k].cpu(), p.grad) for k, p in om.named_parameters()}
    worst = sorted(cos.items(), key=lambda kv: kv[1])[:3]
    print("gradient cosines: median", np.median(list(cos.values())), "worst", worst)
    assert worst[0][1] > 0.99, worst          # fp32 sum-order noise through 53 BatchNorms at N = 2: ~1e-3


def _engine_grads(eng):
    keep = eng.P.data.clone()
    eng.P.data.copy_(eng.G)
    gsd = eng.state_dict()
    eng.P.data.copy_(keep)
    return gsd


class _RoundBF16(torch.autograd.Function):
    """y = bf16(x) forward, bf16(g) backward: what STORING a tensor and its gradient in bf16 does to them"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


def _emulate_bf16_storage(model):
    """ResNet2d with every conv / BatchNorm / ReLU / max-pool output (and its gradient) rounded to bf16: what any correct bf16
    implementation of the step looks like against the fp32 one"""
    return [mod.register_forward_hook(lambda m_, inp, out: _RoundBF16.apply(out)) for mod in model.modules()
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.ReLU, torch.nn.MaxPool2d))]


def _mild_state(om, seed):
    """A state in which the residual network does not amplify (as a trained one): block-final gammas in [0.1, 0.3], every other
    gamma in [0.75, 1.25], betas ~ N(0, 0.1), non-trivial running statistics, filters both precisions hold exactly."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in om.state_dict().items():
            if k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)
            elif k.endswith("bn3.weight"):
                v.copy_(torch.rand(v.shape, generator=g) * 0.2 + 0.1)
            elif (".bn" in k or k.startswith("bn1") or "downsample.1" in k) and k.endswith("weight"):
                v.copy_(torch.rand(v.shape, generator=g) * 0.5 + 0.75)
            elif (".bn" in k or k.startswith("bn1") or "downsample.1" in k) and k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
            elif v.dim() == 4:                             # the 53 Conv2d filters
                v.copy_(v.to(torch.bfloat16).float())


@pytest.mark.parametrize("n,crop", [(2, 128), (8, 128), (4, 192)])
def test_model_bf16_step_against_bf16_storage_yardstick(n, crop):
    """bf16 engine (the stem2d kernels, then the trunk's bf16-only kernels at T = 1) against ResNet2d fp32 on the same
    bf16-representable clips and filters, measured against the yardstick of ResNet2d itself with bf16 storage emulated:
    the engine may lose what bf16 storage costs and nothing more."""
    from video_classification_amd.slowfast import resnet50_2d_engine
    torch.manual_seed(0)
    om = resnet50_2d(50, 1000)
    _mild_state(om, 3)
    sd0 = {k: v.clone() for k, v in om.state_dict().items()}
    m = resnet50_2d_engine(1000, 10, crop, dtype=torch.bfloat16, device=DEV, backend=HipBackend())
    m.load_state_dict(sd0, strict=True)
    clips = torch.randn(n, 10, 21, crop, crop, generator=torch.Generator().manual_seed(crop + n)).to(torch.bfloat16).float()
    x = clips[:, :, :5].reshape(n, 50, crop, crop)
    labels = torch.arange(n) * 131 % 1000
    om.train()
    y_o = om(x)
    loss_o = torch.nn.functional.cross_entropy(y_o, labels)
    loss_o.backward()
    ref = {k: p.grad.clone() for k, p in om.named_parameters()}
    osd = {k: v.clone() for k, v in om.state_dict().items()}
    om.load_state_dict(sd0)
    om.zero_grad()
    hooks = _emulate_bf16_storage(om)
    y_e = om(x)
    torch.nn.functional.cross_entropy(y_e, labels).backward()
    for h in hooks:
        h.remove()
    emu = {k: p.grad.clone() for k, p in om.named_parameters()}
    m.train()
    y_m = m(clips.to(DEV)[:, :, :5])
    loss_m = torch.nn.functional.cross_entropy(y_m, labels.to(DEV))
    loss_m.backward()
    gsd = _engine_grads(m.engine)

    def cosines(grads):
        return sorted((cosine(grads[k].cpu(), r), float(grads[k].norm() / (r.norm() + 1e-30)), k) for k, r in ref.items())
    rows, rows_e = cosines(gsd), cosines(emu)
    cos, cos_e = np.array([r[0] for r in rows]), np.array([r[0] for r in rows_e])
    fwd, fwd_e = rel_err(y_m.detach().float().cpu(), y_o.detach()), rel_err(y_e.detach(), y_o.detach())
    msd = m.state_dict()
    rv = max(rel_err(msd[k].cpu(), osd[k]) for k in osd if k.endswith(("running_mean", "running_var")))
    print(f"res2d bf16 N={n} S={crop}: logits {fwd:.2e} (bf16-storage ResNet2d {fwd_e:.2e}), loss {float(loss_m.detach()):.4f} vs "
          f"{float(loss_o):.4f}, running stats {rv:.2e}; gradient cosine median {np.median(cos):.4f} p10 "
          f"{np.percentile(cos, 10):.4f} worst {rows[0][:3]} | yardstick median {np.median(cos_e):.4f} p10 "
          f"{np.percentile(cos_e, 10):.4f} worst {rows_e[0][:3]}")
    # (1000 classes: the yardstick's own logits error is 0.9 .. 1.4e-2 at these sizes; the bar is relative to it)
    assert fwd < 3e-2 and fwd < 3.0 * fwd_e + 1e-3, (fwd, fwd_e)
    assert abs(float(loss_m.detach()) - float(loss_o.detach())) < 5e-3 * float(loss_o.detach())
    assert rv < 1e-2, rv
    assert np.median(cos) > 0.90 and np.percentile(cos, 10) > 0.85 and cos.min() > 0.6, (np.median(cos), rows[:5])
    assert np.median(cos) > np.median(cos_e) - 0.03 and np.percentile(cos, 10) > np.percentile(cos_e, 10) - 0.05
    assert all(0.4 < r[1] < 2.0 for r in rows), [r for r in rows if not 0.4 < r[1] < 2.0][:5]


def test_full_batch_bf16_trains_and_graph_replay_equals_eager():
    """res2d.yaml geometry: N = 60, T = 10, CropTorso 128, bf16.  Five fused steps on one batch lower the loss; the same five
    steps replayed from a captured hipGraph (single-stream schedule) give the same losses."""
    from video_classification_amd.slowfast import resnet50_2d_engine
    from video_classification_amd.train import TrainStep
    g = torch.Generator().manual_seed(60)
    clips = torch.randn(60, 10, 21, 128, 128, generator=g).to(DEV)
    labels = torch.randint(0, 1000, (60,), generator=g).to(DEV)
    losses = {}
    for use_graph in (False, True):
        m = resnet50_2d_engine(1000, 10, 128, dtype=torch.bfloat16, device=DEV, backend=HipBackend(), seed=3)
        m.engine.two_streams = False
        m.train()
        step = TrainStep(m.engine, lr=1e-3, use_graph=use_graph)
        ls = []
        for _ in range(5):
            ls.append(float(step(clips[:, :, :5], None, labels)))
        torch.cuda.synchronize()
        losses[use_graph] = ls
        if use_graph:
            assert any(e["graph"] is not None for e in step._cache.values())
    print("losses eager", losses[False], "graph", losses[True])
    ls = losses[False]
    assert all(np.isfinite(ls)) and ls[-1] < ls[0] and abs(ls[0] - np.log(1000)) < 1.0, ls
    assert np.allclose(losses[True], losses[False], rtol=2e-2, atol=0), losses


def test_trainer_engine_backend_end_to_end(tmp_path):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer, TrainStep
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.CHALEARN.BATCH_SIZE = 4
    cfg.CHALEARN.CLIP_LEN = 10
    cfg.CHALEARN.NUM_CLASS = 5
    cfg.MODEL.NAME = "res2d"
    cfg.MODEL.R3D_INPUT = "CropLHandArm"                    # 128 x 128
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.DTYPE = "bf16"
    cfg.NUM_CPU = 0
    tr = SyntheticChalearn(cfg, "train", num_videos=8, seed=1)
    te = SyntheticChalearn(cfg, "test", num_videos=3, clips_per_video=(1, 3), seed=2)
    t = Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    assert isinstance(t.step, TrainStep) and t.model.engine.dtype == torch.bfloat16
    loss, _ = t.train_epoch()
    assert np.isfinite(loss)
    res = t.run_eval()
    assert res["ps"].shape == (sum(te.nclips), 1000) and np.allclose(res["ps"].sum(1), 1.0, atol=1e-4)
    t.save_ckpt(epoch=0, acc=float(res["acc"]))
    ckpts = sorted(t.ckpt_dir.glob("*"))
    assert ckpts
    ref = ResNet2d((3, 4, 6, 3), 50, 1000)
    ref.load_state_dict(torch.load(ckpts[-1], map_location="cpu", weights_only=True), strict=True)
