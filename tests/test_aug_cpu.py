"""The device-side ColorJitter on CPU (include/sfk_aug.h, input_pipeline.draw_color_jitter / ColorJitter, tests/ref_jitter.py,
tests/emu_aug.py): the ctypes binding of the new header and its host-side rejections, the parameter draws against a literal
transcription of torchvision's ColorJitter.get_params, properties of the restated transform, and the wiring of the optional
'jitter' batch entry through both ModelManagers and the datasets."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from emu_aug import EmuAugBackend
from emu_v2 import roi_resize_ref
from ref_jitter import ref_jitter
from video_classification_amd import gesture_v2 as v2
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import byte_lut, draw_color_jitter, normalize_lut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the binding of include/sfk_aug.h
def test_aug_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_aug.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_AUG) == ["sfk_aug_abi_version", "sfk_color_jitter", "sfk_color_jitter_workspace_bytes"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_AUG[n]), n
    assert lib.sfk_aug_abi_version() == _lib.AUG_ABI_VERSION == int(re.search(r"#define\s+SFK_AUG_ABI_VERSION\s+(\d+)", src).group(1))
    assert lib.sfk_color_jitter_workspace_bytes.restype is ctypes.c_int64
    # the struct: field names in order, C sizes of their types
    body = re.search(r"typedef struct \{(.*?)\} sfk_jitter_desc;", src, flags=re.S).group(1)
    fields, sizes = [], {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "float": 4}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(3).replace("*", "").split(","):
            fields.append((nm.strip(), 8 if m.group(2) else sizes[m.group(1)]))
    assert [(f, ctypes.sizeof(t)) for f, t in _lib._JitterDesc._fields_] == fields
    assert [f for f, _ in fields] == ["struct_size", "dtype", "x", "sn", "st", "sc", "sh", "n", "t", "h", "w", "c_off", "bgr",
                                      "mean", "std", "params", "workspace"]
    assert ctypes.sizeof(_lib._JitterDesc) == 96 == _lib.new_jitter_desc().struct_size


def _good_jitter(x, params, ws):
    from video_classification_amd import _lib
    d = _lib.new_jitter_desc()
    d.dtype, d.x, d.params, d.workspace = _lib.SFK_F32, x.data_ptr(), params.data_ptr(), ws.data_ptr()
    d.n, d.t, d.h, d.w = 2, 3, 16, 24
    d.sn, d.st, d.sc, d.sh = 3 * 7 * 16 * 24, 7 * 16 * 24, 16 * 24, 24
    d.c_off, d.bgr, d.mean, d.std = 0, 0, 0.0, 1.0
    return d


def test_aug_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    x, params, ws = torch.zeros(2 * 3 * 7 * 16 * 24), torch.zeros(2, 8), torch.zeros(64)
    before = (x.clone(), params.clone(), ws.clone())
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 92), ("struct_size", 104), ("x", None), ("params", None),
                         ("workspace", None), ("n", 0), ("t", -1), ("h", 0), ("w", -3), ("sn", -1), ("st", -5), ("sc", -1),
                         ("sh", -24), ("c_off", -1), ("bgr", 2), ("bgr", -1), ("std", 0.0), ("std", -0.225),
                         ("std", float("nan")), ("dtype", 2), ("dtype", -1)]:
        d = _good_jitter(x, params, ws)
        setattr(d, field, value)
        assert lib.sfk_color_jitter(B(d), None) == -1, (field, value)
    assert lib.sfk_color_jitter(None, None) == -1
    for field, value in [("h", 8193), ("n", (1 << 23) + 1)]:              # 8193 * 8193 pixels; more frames than workgroups
        d = _good_jitter(x, params, ws)
        setattr(d, field, value)
        if field == "h":
            d.w = 8193
        assert lib.sfk_color_jitter(B(d), None) == -2, field
    assert all(torch.equal(a, b) for a, b in zip(before, (x, params, ws)))
    wb = lib.sfk_color_jitter_workspace_bytes
    assert wb(0, 1, 8, 8) == wb(1, 0, 8, 8) == wb(1, 1, -1, 8) == wb(1, 1, 8, 0) == -1
    assert wb(1, 1, 8193, 8193) == -2 and wb(1 << 22, 4, 8, 8) == -2
    # positive, a whole number of floats, one slot per 512 eight-pixel units of a frame, growing with n * t
    assert wb(1, 1, 1, 1) == 4 and wb(1, 1, 17, 19) == 4 and wb(1, 1, 192, 192) == 9 * 4 and wb(1, 1, 64, 65) == 2 * 4
    assert wb(10, 20, 192, 192) == 200 * 9 * 4 < wb(11, 20, 192, 192) < wb(11, 21, 192, 192)
    be = EmuAugBackend()
    for g in [(1, 1, 1, 1), (3, 2, 17, 19), (10, 20, 192, 192), (2, 2, 64, 65)]:
        assert be.color_jitter_workspace_bytes(*g) == wb(*g)


# ------------------------------------------------------------------ the draws
def get_params_transcribed(brightness, contrast, saturation, hue, generator):
    """torchvision.transforms.ColorJitter.get_params, literally, with every draw taken from `generator`; the arguments are the
    (min, max) ranges of ColorJitter.__init__ / _check_input, None for an op that is off"""
    fn_idx = torch.randperm(4, generator=generator)
    b = None if brightness is None else float(torch.empty(1).uniform_(brightness[0], brightness[1], generator=generator))
    c = None if contrast is None else float(torch.empty(1).uniform_(contrast[0], contrast[1], generator=generator))
    s = None if saturation is None else float(torch.empty(1).uniform_(saturation[0], saturation[1], generator=generator))
    h = None if hue is None else float(torch.empty(1).uniform_(hue[0], hue[1], generator=generator))
    return fn_idx, b, c, s, h


def check_input(value, center=1.0, clip_first_on_zero=True):
    """ColorJitter._check_input for a number: [center - v, center + v], the lower end clipped at 0, None when that is a point"""
    lo, hi = center - float(value), center + float(value)
    if clip_first_on_zero:
        lo = max(lo, 0.0)
    return None if lo == hi == center else (lo, hi)


def test_draws_equal_get_params_on_the_same_generator():
    ga, gb = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    got = draw_color_jitter(50, generator=ga)
    assert got.dtype == torch.float32 and tuple(got.shape) == (50, 8)
    ranges = (check_input(0.5), check_input(0.3), check_input(0.2), check_input(0.1, 0.0, False))
    assert ranges == ((0.5, 1.5), (0.7, 1.3), (0.8, 1.2), (-0.1, 0.1))
    for i in range(50):
        fn_idx, b, c, s, h = get_params_transcribed(*ranges, gb)
        assert got[i, :4].tolist() == fn_idx.tolist()
        assert got[i, 4:].tolist() == [torch.tensor(v, dtype=torch.float32).item() for v in (b, c, s, h)]
    assert torch.equal(torch.empty(1).uniform_(generator=ga), torch.empty(1).uniform_(generator=gb))      # same stream position


def test_draw_ranges_over_1000_draws():
    p = draw_color_jitter(1000, 0.5, 0.3, 0.2, 0.1, torch.Generator().manual_seed(1))
    assert all(sorted(r) == [0, 1, 2, 3] for r in p[:, :4].tolist())
    for col, (lo, hi) in zip(range(4, 8), [(0.5, 1.5), (0.7, 1.3), (0.8, 1.2), (-0.1, 0.1)]):
        v = p[:, col]
        assert lo <= float(v.min()) and float(v.max()) <= hi and float(v.max() - v.min()) > 0.9 * (hi - lo)
    wide = draw_color_jitter(200, 1.5, 0.3, 0.2, 0.5, torch.Generator().manual_seed(2))      # the lower end is clipped at 0
    assert 0.0 <= float(wide[:, 4].min()) < 0.2 and float(wide[:, 4].max()) <= 2.5 and float(wide[:, 7].abs().max()) <= 0.5


def test_zero_range_skips_the_op_and_takes_no_draw():
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    got = draw_color_jitter(40, 0.5, 0.0, 0.2, 0.0, ga)
    ranges = (check_input(0.5), check_input(0.0), check_input(0.2), check_input(0.0, 0.0, False))
    assert ranges[1] is None and ranges[3] is None
    for i in range(40):
        fn_idx, b, c, s, h = get_params_transcribed(*ranges, gb)
        want = [float(k) if k in (0, 2) else -1.0 for k in fn_idx.tolist()]       # contrast (1) and hue (3) are off
        assert got[i, :4].tolist() == want
        assert got[i, 4:].tolist() == [torch.tensor(b, dtype=torch.float32).item(), 1.0,
                                       torch.tensor(s, dtype=torch.float32).item(), 0.0]
    assert torch.equal(torch.empty(1).uniform_(generator=ga), torch.empty(1).uniform_(generator=gb))
    off = draw_color_jitter(3, 0, 0, 0, 0, torch.Generator().manual_seed(0))
    assert off[:, :4].eq(-1).all() and off[:, 4:].tolist() == [[1.0, 1.0, 1.0, 0.0]] * 3


# ------------------------------------------------------------------ the restated transform
def _clip(n=2, t=2, c=3, h=9, w=11, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, t, c, h, w), generator=g).to(dtype) / 255


def _params(rows):
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ref_identity_factors(dtype):
    x = _clip(dtype=dtype)
    p = _params([[0, 1, 2, -1, 1, 1, 1, 0], [2, -1, 1, 0, 1, 1, 1, 0]])
    assert torch.equal(ref_jitter(x, p), x)                      # brightness, contrast, saturation at 1: exact
    p = _params([[0, 1, 2, 3, 1, 1, 1, 0], [3, 2, 1, 0, 1, 1, 1, 0]])
    got = ref_jitter(x, p)                                       # a hue shift of 0 still goes through HSV and back
    assert got.dtype == dtype and float((got - x).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-14)
    y = ref_jitter(x, _params([[-1, -1, -1, -1, 0.5, 0.7, 0.8, 0.1]] * 2))
    assert torch.equal(y, x)                                     # every slot skipped: the factors are not read


def test_ref_contrast_zero_is_the_frame_gray_mean():
    x = _clip(n=1, t=3)
    got = ref_jitter(x, _params([[1, -1, -1, -1, 1, 0, 1, 0]]))
    gray = 0.2989 * x[:, :, 0] + 0.587 * x[:, :, 1] + 0.114 * x[:, :, 2]
    m = gray.mean(dim=(-2, -1))                                  # one mean per frame, not per clip
    assert len(set(m.flatten().tolist())) == 3
    assert torch.allclose(got, m[:, :, None, None, None].expand_as(got), rtol=0, atol=1e-15)


def test_ref_hue_shift_and_back_on_saturated_pixels():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 2, 3, 16, 16, generator=g)
    x[:, :, 0] = x[:, :, 0] * 0.2                                # R small, so max - min >= 0.3 wherever G or B is large
    x[:, :, 1] = 0.5 + x[:, :, 1] * 0.5
    y = ref_jitter(x, _params([[3, -1, -1, -1, 1, 1, 1, 0.3]]))
    assert float((y - x).abs().max()) > 0.1
    z = ref_jitter(y, _params([[3, -1, -1, -1, 1, 1, 1, -0.3]]))
    assert float((z - x).abs().max()) <= 1e-5


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (0.45, 0.225)])
def test_ref_bgr_is_rgb_on_flipped_planes(mean, std):
    x = (_clip(c=5, dtype=torch.float32) - mean) / std
    rows = [list(o) + [1.2, 0.8, 1.1, 0.07] for o in itertools.islice(itertools.permutations(range(4)), 5, 7)]
    p = _params(rows)
    got = ref_jitter(x, p, 1, True, mean, std)
    flipped = x.clone()
    flipped[:, :, 1:4] = x[:, :, 1:4].flip(2)
    want = ref_jitter(flipped, p, 1, False, mean, std)
    want[:, :, 1:4] = want[:, :, 1:4].flip(2)
    assert torch.equal(got, want)
    assert torch.equal(got[:, :, 0], x[:, :, 0]) and torch.equal(got[:, :, 4], x[:, :, 4])
    assert not torch.equal(got[:, :, 1:4], x[:, :, 1:4])


# ------------------------------------------------------------------ the wiring
def _cfg(t=4, size=64, bs=2, jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = t
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "gesture-v2"
    cfg.MODEL.INPUT_SIZE = size
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


def test_config_defaults():
    from video_classification_amd.config import get_cfg
    m = get_cfg().MODEL
    assert m.COLOR_JITTER is False
    assert (m.JITTER_BRIGHTNESS, m.JITTER_CONTRAST, m.JITTER_SATURATION, m.JITTER_HUE) == (0.5, 0.3, 0.2, 0.1)
    assert v1.jitter_ranges(get_cfg()) is None and v1.jitter_ranges(_cfg(jitter=True)) == (0.5, 0.3, 0.2, 0.1)


def test_v2_prepare_data_with_and_without_jitter():
    g = torch.Generator().manual_seed(2)
    jit = draw_color_jitter(2, generator=g)
    ub = {"frames_u8": torch.randint(0, 256, (2, 4, 48, 64, 7), generator=g, dtype=torch.uint8),
          "box": torch.tensor([[0, 0, 64, 48], [10, 3, 30, 40]], dtype=torch.int32),
          "crop": torch.tensor([[0, 5], [12, 3]], dtype=torch.int32), "label": torch.tensor([1, 5])}
    mm = v2.ModelManager(_cfg(), "cpu", EmuAugBackend())
    (ps, pf), _ = mm.prepare_data(ub)
    plain = roi_resize_ref(ub["frames_u8"], byte_lut(), ub["box"], 64, 64, True, ub["crop"], 6).permute(0, 2, 1, 3, 4)
    assert torch.equal(ps, plain[:, :5]) and torch.equal(pf, plain[:, 5:])                   # today's output, bit for bit
    (js, jf), _ = mm.prepare_data(dict(ub, jitter=jit))
    assert js.untyped_storage().data_ptr() == jf.untyped_storage().data_ptr()
    assert torch.equal(js[:, 3:5], ps[:, 3:5]) and torch.equal(jf, pf)                       # U, V and the flow: untouched
    want = ref_jitter(plain.permute(0, 2, 1, 3, 4).contiguous(), jit)                        # after the resize and the crop
    assert torch.equal(js[:, :3], want.permute(0, 2, 1, 3, 4)[:, :3]) and not torch.equal(js[:, :3], ps[:, :3])
    # the float batch: 'rgb' jittered on the device copy, the loader's tensors left as they are
    fb = {"rgb": torch.rand(2, 4, 3, 64, 64, generator=g), "uv": torch.rand(2, 4, 2, 64, 64, generator=g),
          "flow": torch.rand(2, 4, 2, 64, 64, generator=g), "label": torch.tensor([1, 5])}
    keep = fb["rgb"].clone()
    (fs, ff), _ = mm.prepare_data(fb)
    assert torch.equal(fs[:, :3], fb["rgb"].permute(0, 2, 1, 3, 4))
    (gs, gf), _ = mm.prepare_data(dict(fb, jitter=jit))
    assert torch.equal(fb["rgb"], keep)
    assert torch.equal(gs[:, :3], ref_jitter(fb["rgb"], jit).permute(0, 2, 1, 3, 4))
    assert torch.equal(gs[:, 3:], fs[:, 3:]) and torch.equal(gf, ff)


def _v1_cfg(name="slowfast-LHand", u8_stem=False):
    cfg = _cfg()
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.U8_STEM = u8_stem
    return cfg


def _v1_u8_batch():
    g = torch.Generator().manual_seed(4)
    return {"CropLHand_u8": torch.randint(0, 256, (2, 3, 64, 64, 21), generator=g, dtype=torch.uint8),
            "crop": torch.tensor([[0, 12], [7, 3]], dtype=torch.int32), "label": torch.tensor([0, 3])}, draw_color_jitter(2, generator=g)


@pytest.mark.parametrize("name", ["slowfast-LHand", "res3d"])
def test_v1_prepare_data_with_and_without_jitter(name):
    ub, jit = _v1_u8_batch()
    mm = v1.ModelManager(_v1_cfg(name), "cpu", EmuAugBackend())
    x0, _ = mm.prepare_data(ub)
    x1, _ = mm.prepare_data(dict(ub, jitter=jit))
    if name == "res3d":
        x0, x1 = [x0], [x1]
    # today's output: the table lookup of every byte, shifted by the crop
    from video_classification_amd.input_pipeline import DevicePreprocess
    plain = DevicePreprocess("cpu", EmuAugBackend())(ub["CropLHand_u8"], ub["crop"])          # (N, T, 21, S, S)
    assert torch.equal(x0[0], plain.permute(0, 2, 1, 3, 4)[:, :5])
    assert float(plain[0, 0, :, 0, 0].abs().max()) == 0 and float(normalize_lut()[0]) == -2.0     # the padding is stored 0
    want = ref_jitter(plain, jit, 0, True, 0.45, 0.225).permute(0, 2, 1, 3, 4)                # B, G, R planes, image values
    assert torch.equal(x1[0][:, :3], want[:, :3]) and not torch.equal(x1[0][:, :3], x0[0][:, :3])
    assert torch.equal(x1[0][:, 3:], x0[0][:, 3:])
    if name != "res3d":
        assert torch.equal(x1[1], x0[1]) and torch.equal(x0[1], plain.permute(0, 2, 1, 3, 4)[:, 5:20])
    # the float32 loader batch
    fb = {"CropLHand": plain.clone(), "label": ub["label"]}
    y1, _ = mm.prepare_data(dict(fb, jitter=jit))
    y1 = y1 if name == "res3d" else y1[0]
    assert torch.equal(fb["CropLHand"], plain) and torch.equal(y1[:, :3], want[:, :3]) and torch.equal(y1[:, 3:], x0[0][:, 3:])


def test_u8_stem_with_jitter_is_an_error():
    ub, jit = _v1_u8_batch()
    mm = v1.ModelManager(_v1_cfg(u8_stem=True), "cpu", EmuAugBackend())
    mm.prepare_data(ub)                                                       # the uint8 stems alone are fine
    with pytest.raises(ValueError, match=r"U8_STEM.*jitter|jitter.*U8_STEM"):
        mm.prepare_data(dict(ub, jitter=jit))


def _same_item(a, b):
    return a.keys() == b.keys() and all(torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])) for k in a)


@pytest.mark.parametrize("as_uint8", [False, True])
def test_synthetic_chalearn_attaches_the_key_to_train_items_only(as_uint8):
    off, on = _v1_cfg(), _v1_cfg()
    on.MODEL.COLOR_JITTER = True
    on.MODEL.JITTER_HUE = 0.0
    for name in ("train", "test"):
        a = v1.SyntheticChalearn(off, name, num_videos=3, seed=1, as_uint8=as_uint8)
        b = v1.SyntheticChalearn(on, name, num_videos=3, seed=1, as_uint8=as_uint8)
        for i in range(3):
            ia, ib = (a[i], b[i]) if name == "train" else (a[i][0], b[i][0])
            assert "jitter" not in ia
            if name == "test":
                assert all(_same_item(p, q) for p, q in zip(a[i], b[i]))
                continue
            jit = ib.pop("jitter")
            assert _same_item(ia, ib)                                         # everything else is what it is with the key off
            assert jit.dtype == torch.float32 and tuple(jit.shape) == (8,) and float(jit[7]) == 0.0 and -1.0 in jit[:4].tolist()
            assert 0.5 <= float(jit[4]) <= 1.5 and torch.equal(jit, b[i]["jitter"])


def test_synthetic_gesture_and_gesture_frames_attach_the_key_to_train_items_only(tmp_path):
    from test_v2_cpu import _fake_tree
    off, on = _cfg(), _cfg(jitter=True)
    for name in ("train", "test"):
        a = v2.SyntheticGesture(off, name, num_videos=2, seed=1, h=24, w=32, min_box=8)
        b = v2.SyntheticGesture(on, name, num_videos=2, seed=1, h=24, w=32, min_box=8)
        ia, ib = (a[0], b[0]) if name == "train" else (a[0][0], b[0][0])
        assert "jitter" not in ia and ("jitter" in ib) == (name == "train")
        ib.pop("jitter", None)
        assert _same_item(ia, ib)
    cfg, labels, read_video, _ = _fake_tree(tmp_path, [(40, [4, 15, 1])])
    parts = v2.PartCompose.lHandArmTorso
    assert "jitter" not in v2.ChalearnGestureFrames(cfg, "train", parts, "random", labels, read_video)[0]
    cfg.MODEL.COLOR_JITTER = True
    it = v2.ChalearnGestureFrames(cfg, "train", parts, "random", labels, read_video)[0]
    assert tuple(it["jitter"].shape) == (8,) and sorted(it["jitter"][:4].tolist()) == [0, 1, 2, 3]
    assert all("jitter" not in c for c in v2.ChalearnGestureFrames(cfg, "test", parts, "uniform", labels, read_video)[0])
    assert all("jitter" not in c for c in v2.ChalearnGestureFrames(cfg, "train", parts, "uniform", labels, read_video)[0])
    assert "jitter" not in v2.ChalearnGestureFrames(cfg, "test", parts, "random", labels, read_video)[0]


def test_v2_trainer_epoch_with_color_jitter(tmp_path):
    import math
    cfg = _cfg(jitter=True)
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.MODEL.LR = 1e-2
    tr = v2.SyntheticGesture(cfg, "train", num_videos=3, seed=1, h=48, w=64, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuAugBackend())
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append(tuple(batch["jitter"].shape)), prepare(batch))[1]
    loss, _ = t.train_epoch()
    assert seen == [(2, 8), (1, 8)] and math.isfinite(loss)
    assert sorted(t.mm.color_jitter()._ws) == [(1, 4, 64, 64), (2, 4, 64, 64)]             # one workspace per geometry
