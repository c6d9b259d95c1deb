"""The res2d network (torchvision ResNet-50 over T frames x 5 channels stacked on conv1's input, reference train.py:64-76) on
the engine's schedule, against res2d.py's torch.nn ResNet2d (same state dict), on CPU: the frames-as-channels stem runs as
the torch restatement of include/sfk_stem2d.h (tests/emu_stem2d.py).  Also: the checkpoint surface, the trainer's backend
key and the ctypes binding of the new header."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from emu_stem2d import EmuStem2dBackend
from helpers import rel_err, rel_l2
from video_classification_amd import arch
from video_classification_amd.res2d import ResNet2d, resnet50_2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_var") or (".bn" in "." + k and k.endswith("weight")) or (k.startswith("bn1") and k.endswith("weight")) \
                    or (k.endswith("downsample.1.weight")):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean") or k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)
            elif k == "fc.weight":
                v.copy_(torch.randn(v.shape, generator=g) * 0.05)


def make_pair(t, num_class=7, crop=64, depth=18, seed=11):
    from video_classification_amd.slowfast import resnet50_2d_engine
    torch.manual_seed(seed)
    om = ResNet2d(arch.STAGE_DEPTHS[depth], 5 * t, num_class)
    randomize(om, seed)
    m = resnet50_2d_engine(num_class, t, crop, dtype=torch.float32, device="cpu", backend=EmuStem2dBackend(), depth=depth)
    m.load_state_dict(om.state_dict(), strict=True)
    return om, m


def loader_batch(n, t, s, seed=3):
    return torch.randn(n, t, 21, s, s, generator=torch.Generator().manual_seed(seed))


def reshape_input(clips):
    x = clips[:, :, :5]
    n, t, c, h, w = x.shape
    return torch.reshape(x, (n, t * c, h, w))


def grads_as_state_dict(eng):
    keep = eng.P.data.clone()
    eng.P.data.copy_(eng.G)
    gsd = eng.state_dict()
    eng.P.data.copy_(keep)
    return gsd


@pytest.mark.parametrize("t", [2, 10])
def test_forward_and_train_step_match_resnet2d(t):
    om, m = make_pair(t)
    clips = loader_batch(2, t, 64)
    x = reshape_input(clips)
    om.eval(); m.eval()
    with torch.no_grad():
        want = om(x)
    assert rel_err(m(x), want) < 1e-4
    # one training step: loss, every parameter gradient, the running statistics
    om.train(); m.train()
    labels = torch.tensor([1, 5])
    loss_o = torch.nn.functional.cross_entropy(om(x), labels)
    loss_o.backward()
    y_m = m(clips[:, :, :5])                          # the loader's view, read in place
    loss_m = torch.nn.functional.cross_entropy(y_m, labels)
    loss_m.backward()
    assert abs(float(loss_m) - float(loss_o)) < 1e-4
    gsd = grads_as_state_dict(m.engine)
    for k, p in om.named_parameters():
        assert rel_l2(gsd[k], p.grad) < 1e-3, k
    osd, msd = om.state_dict(), m.state_dict()
    for k in osd:
        if k.endswith(("running_mean", "running_var")):
            assert rel_err(msd[k], osd[k]) < 1e-4, k


def test_state_dict_surface_is_torchvision_resnet50():
    from video_classification_amd.engine import Engine
    e = Engine(arch.resnet2d_spec(1000, 10), dtype=torch.float32, device="cpu", backend=EmuStem2dBackend())
    ref = resnet50_2d(50, 1000)
    sd_r, sd_e = ref.state_dict(), e.state_dict()
    assert list(sd_e) == list(sd_r) or set(sd_e) == set(sd_r)
    for k in sd_r:
        assert tuple(sd_e[k].shape) == tuple(sd_r[k].shape), k
    assert tuple(sd_e["conv1.weight"].shape) == (64, 50, 7, 7) and tuple(sd_e["fc.weight"].shape) == (1000, 2048)
    assert e.num_parameters() == sum(p.numel() for p in ref.parameters())
    randomize(ref, 5)
    e.load_state_dict(ref.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(e.state_dict()[k].to(v.dtype), v), k
    back = resnet50_2d(50, 1000)
    back.load_state_dict(e.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


def test_strided_loader_view_equals_the_reshape():
    om, m = make_pair(10)
    clips = loader_batch(2, 10, 64, seed=9)
    m.eval()
    with torch.no_grad():
        a = m(reshape_input(clips)).clone()
        b = m(clips[:, :, :5]).clone()
        c = m(clips).clone()                                    # (N, T, 21, S, S): the stem reads channels 0..4
    assert torch.equal(a, b) and torch.equal(a, c)
    v = m.engine.input_view(clips[:, :, :5])
    assert v.data_ptr() == clips.data_ptr() and tuple(v.shape) == (2, 5, 10, 64, 64)


def _cfg(tmp_path, backend):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 2
    cfg.CHALEARN.NUM_CLASS = 5
    cfg.MODEL.NAME = "res2d"
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.LR = 1e-3
    cfg.NUM_CPU = 0
    cfg.DEBUG = True
    if backend is not None:
        cfg.MODEL.RES2D_BACKEND = backend
    return cfg


def test_trainer_backend_key(tmp_path):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.slowfast import SlowFast
    from video_classification_amd.train import ModelManager, SyntheticChalearn, Trainer, TrainStep
    from video_classification_amd.res2d import TorchStep
    assert get_cfg().MODEL.RES2D_BACKEND == "torch"
    cfg = _cfg(tmp_path, None)
    assert isinstance(ModelManager(cfg, device="cpu").init_model(), ResNet2d)
    cfg = _cfg(tmp_path, "engine")
    mm = ModelManager(cfg, device="cpu", backend=EmuStem2dBackend())
    model = mm.init_model()
    assert isinstance(model, SlowFast) and model.spec.frames_as_channels and model.engine.dtype == torch.float32
    tr = SyntheticChalearn(cfg, "train", num_videos=2, seed=1)
    te = SyntheticChalearn(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2)
    t = Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuStem2dBackend())
    assert isinstance(t.step, TrainStep)
    x, y = t.mm.prepare_data(next(iter(t.train_loader)))
    assert tuple(x.shape) == (2, 2, 5, 64, 64) and x.stride(1) == 21 * 64 * 64      # no reshape copy
    loss, _ = t.train_epoch()
    assert loss == loss
    res = t.run_eval()
    assert res["ps"].shape[1] == 1000
    ref = resnet50_2d(10, 1000)
    ref.load_state_dict(t.model.state_dict(), strict=True)
    t2 = Trainer(_cfg(tmp_path, None), train_set=tr, test_set=te, device="cpu")
    assert isinstance(t2.step, TorchStep)
    t.model.load_state_dict(t2.model.state_dict(), strict=True)
    with pytest.raises(ValueError):
        ModelManager(_cfg(tmp_path, "nope"), device="cpu").init_model()


# ------------------------------------------------------------------ the binding of include/sfk_stem2d.h
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def test_stem2d_table_matches_its_header(lib):
    from video_classification_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfk_stem2d.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert len(names) == 4
    assert sorted(_lib.SIGNATURES_STEM2D) == names
    assert not set(names) & set(_lib.SIGNATURES)
    for n in names:
        assert hasattr(lib, n)
    # prototype arity
    for n in names:
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_STEM2D[n]), n
    assert lib.sfk_stem2d_abi_version() == _lib.STEM2D_ABI_VERSION == int(
        re.search(r"#define\s+SFK_STEM2D_ABI_VERSION\s+(\d+)", src).group(1))
    assert ctypes.sizeof(_lib._Stem2dSrc) == 80


def test_stem2d_rejects_bad_descriptors_on_the_host(lib):
    from video_classification_amd import _lib
    d = _lib.new_stem2d_src()
    y = _lib._FMap()
    assert lib.sfk_stem2d_fwd(ctypes.byref(d), None, ctypes.byref(y), None, None) == -1       # null pointers
    assert lib.sfk_stem2d_wgrad(ctypes.byref(d), ctypes.byref(y), None, None) == -1
    assert lib.sfk_stem2d_tiles(None, None) == -1
    buf = torch.zeros(64, dtype=torch.float32)
    d.src, d.src_dtype = buf.data_ptr(), _lib.SFK_F32
    d.sn, d.st, d.sc, d.sh, d.sw = 5 * 2 * 64 * 64, 5 * 64 * 64, 64 * 64, 64, 1
    d.n, d.t, d.c, d.h_in, d.w_in = 3, 2, 5, 64, 64
    y.ptr, y.dtype = buf.data_ptr(), _lib.SFK_F32
    y.n, y.t, y.h, y.w, y.c, y.ld, y.c_off = 3, 1, 32, 32, 64, 64, 0
    assert lib.sfk_stem2d_tiles(ctypes.byref(d), ctypes.byref(y)) == 3 * 2 * 2
    y.h = 31                                                                                  # ho mismatch
    assert lib.sfk_stem2d_fwd(ctypes.byref(d), buf.data_ptr(), ctypes.byref(y), None, None) == -1
    y.h, y.w = 32, 33
    assert lib.sfk_stem2d_wgrad(ctypes.byref(d), ctypes.byref(y), buf.data_ptr(), None) == -1
    y.w, y.c, y.ld = 32, 62, 62                                                                # cout % 4
    assert lib.sfk_stem2d_fwd(ctypes.byref(d), buf.data_ptr(), ctypes.byref(y), None, None) == -2
    y.c, y.ld = 128, 128                                                                       # cout > 64
    assert lib.sfk_stem2d_wgrad(ctypes.byref(d), ctypes.byref(y), buf.data_ptr(), None) == -2
    y.c, y.ld = 64, 64
    d.struct_size = 8                                                                          # other layout
    assert lib.sfk_stem2d_tiles(ctypes.byref(d), ctypes.byref(y)) == -1


def test_main_abi_lock_matches_header():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_lock.py")], capture_output=True, text=True)
    assert out.returncode == 0 and "ABI 24 matches" in out.stdout, out.stdout + out.stderr
