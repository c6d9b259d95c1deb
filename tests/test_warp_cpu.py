"""The random affine augmentation without a GPU (include/sfk_warp.h, input_pipeline.draw_affine, MODEL.AFFINE): the contract
in float32 (tests/ref_warp.py warp32) against F.grid_sample in float64 under a derived bound; the crop as its special case,
bit for bit; exact matrices; the draws; the whole pipeline through the emulation (tests/emu_warp.py); the header's ABI and
host-side rejections through the built library (they launch nothing); and five mutants of the emulation, each refused by the
checks the GPU test runs (ref_warp.check)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import ref_warp as R
from emu_resident import pool_gather_crop
from emu_warp import EmuWarpBackend
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import (DevicePreprocess, FramePool, ResidentTrainSet, affine_forward, affine_inverse,
                                                     draw_affine, draw_affine_params, draw_crop_offsets, identity_warp_rows,
                                                     normalize_lut, validate_warp_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "CropLHand"                                                               # 64 x 64 crops
LUT = normalize_lut()
WILD = dict(degrees=30.0, scale=(0.6, 1.6), shear=10.0, flip=0.5)


def _pool(f, h, w, p=21, seed=0):
    return torch.randint(0, 256, (f, h, w, p), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ------------------------------------------------------------------ warp32 against grid_sample in float64
@pytest.mark.parametrize("s", [17, 32, 192, 224])
def test_warp32_is_grid_sample_within_the_derived_bound(s):
    g = torch.Generator().manual_seed(s)
    pool = _pool(3, s, s, seed=s)
    warp = draw_affine(4, s, s // 10, generator=g, **WILD)
    index = torch.tensor([[0, 1], [2, -1], [1, 1], [0, 2]], dtype=torch.int32)
    got, want = R.warp32(pool, index, LUT, 127, warp), R.warp64(pool, index, LUT, 127, warp)
    err, bound = float((got.double() - want).abs().max()), R.bound(warp, s, s, LUT)
    cx, cy = R.coords64(warp, s, s)[2:]
    print(f"S {s}: worst error {err:.3e}, bound {bound:.3e} at |coordinates| up to {max(cx, cy):.1f}")
    assert got.abs().max() > 1 and err <= bound                               # every element of every clip is compared
    if max(cx, cy) < 512:
        assert bound <= 4.2e-4


def test_the_bound_is_the_stated_formula():
    d = float(LUT[255] - LUT[0])
    assert R.half_ulp(300.0) == 2.0 ** -16 and R.half_ulp(511.9) == 2.0 ** -16 and R.half_ulp(512.0) == 2.0 ** -15
    ident = identity_warp_rows(1)
    assert R.bound(ident, 192, 192, LUT) == 3 * d * 2 * 2.0 ** (7 - 24) + 9 * 2.0 ** -24 * d      # coordinates up to 191


# ------------------------------------------------------------------ the crop is identity plus integer translation
def test_integer_translation_rows_are_the_crop_gather_bit_for_bit():
    s, pad = 32, 3
    pool = _pool(3, s, s, seed=1)
    index = torch.tensor([[0, -1], [2, 1]], dtype=torch.int32)               # a missing frame too
    for top in range(2 * pad + 1):
        for left in range(2 * pad + 1):
            rows = torch.tensor([[1.0, 0.0, left - pad, 0.0, 1.0, top - pad]] * 2)
            crop = torch.tensor([[top, left]] * 2, dtype=torch.int32)
            assert torch.equal(R.warp32(pool, index, LUT, 127, rows), pool_gather_crop(pool, index, LUT, 127, crop, pad, 0, 21)), (top, left)


@pytest.mark.parametrize("s", [192, 224])
def test_integer_translation_rows_at_the_production_sizes(s):
    pad = s // 10
    pool = _pool(2, s, s, p=5, seed=s)
    index = torch.tensor([[1], [-1]], dtype=torch.int32)
    for top, left in [(0, 2 * pad), (2 * pad, 0), (pad + 1, pad - 1)]:
        rows = torch.tensor([[1.0, 0.0, left - pad, 0.0, 1.0, top - pad]] * 2)
        crop = torch.tensor([[top, left]] * 2, dtype=torch.int32)
        assert torch.equal(R.warp32(pool, index, LUT, 127, rows), pool_gather_crop(pool, index, LUT, 127, crop, pad, 0, 5)), (top, left)


# ------------------------------------------------------------------ exact matrices
def test_exact_matrices():
    h = w = 24
    pool = _pool(2, h, w, seed=3)
    index = torch.tensor([[0, 1]], dtype=torch.int32)
    plain = LUT[pool.long()].permute(0, 3, 1, 2)[None]                          # (1, 2, 21, h, w): the normalised frames
    one = lambda row: R.warp32(pool, index, LUT, 127, torch.tensor([row], dtype=torch.float32))
    assert torch.equal(one([1, 0, 0, 0, 1, 0]), plain)
    assert torch.equal(one([-1, 0, w - 1, 0, 1, 0]), plain.flip(-1))           # the horizontal flip
    assert torch.equal(one([0, 1, 0, 1, 0, 0]), plain.transpose(-1, -2))       # the transpose of a square frame
    right = torch.cat([plain[..., 1:], torch.zeros_like(plain[..., :1])], -1)  # the neighbour at x + 1, zero past the edge
    assert torch.equal(one([1, 0, 0.5, 0, 1, 0]), plain + 0.5 * (right - plain))
    up = torch.cat([torch.zeros_like(plain[..., :1, :]), plain[..., :-1, :]], -2)   # ys = y - 0.5: rows y - 1 and y
    assert torch.equal(one([1, 0, 0, 0, 1, -0.5]), up + 0.5 * (plain - up))


def test_far_out_and_non_finite_rows_give_zeros_in_the_emulation():
    """a pure scale keeps its fixed point inside the frame, so the far-out scales of 1e-6 and 1e6 come with a far translation"""
    pool = _pool(2, 24, 40, seed=4)
    index = torch.tensor([[0, 1]], dtype=torch.int32)
    inf, nan = float("inf"), float("nan")
    rows = R.FAR + [[nan, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, nan], [inf, 0, 0, 0, 1, 0], [1, 0, -inf, 0, 1, 0], [1, inf, 0, 0, -inf, 0],
                    [nan] * 6, [3e38, 3e38, 3e38, -3e38, -3e38, 0]]
    be = EmuWarpBackend()
    for row in rows:
        out = torch.full((1, 2, 21, 24, 40), -7.0)
        be.u8_pool_gather_warp(pool, index, LUT, 127, torch.tensor([row], dtype=torch.float32), out)(0)
        assert not out.any(), row
    for row in rows[len(R.FAR):-1]:                                            # (the last row overflows but is finite itself)
        with pytest.raises(ValueError, match="not finite"):
            validate_warp_rows(torch.tensor([[1, 0, 0, 0, 1, 0], row], dtype=torch.float32))
    with pytest.raises(ValueError, match=r"\(n, 6\)"):
        validate_warp_rows(torch.zeros(2, 5))
    ok = validate_warp_rows(torch.tensor(R.FAR, dtype=torch.float64))
    assert ok.dtype == torch.float32 and ok.is_contiguous() and torch.equal(identity_warp_rows(2), torch.tensor([[1., 0, 0, 0, 1, 0]] * 2))


# ------------------------------------------------------------------ draw_affine
def test_degenerate_ranges_reproduce_the_crop_draws():
    """a clip's first two draws are the crop's (every clip of a plan has a generator of its own); the four that follow move
    the stream, so only the first clip of a longer call meets draw_crop_offsets' pair"""
    for s in (64, 192):
        pad = s // 10
        for seed in range(6):
            row = draw_affine(1, s, pad, generator=torch.Generator().manual_seed(seed))[0]
            top, left = draw_crop_offsets(1, pad, torch.Generator().manual_seed(seed))[0].tolist()
            assert row.dtype == torch.float32 and row.tolist() == [1.0, 0.0, left - pad, 0.0, 1.0, top - pad]
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert draw_affine_params(6, generator=g1, **WILD)[:2] == tuple(draw_crop_offsets(1, 6, g2)[0].tolist())


def test_the_stream_position_after_a_row_is_the_same_for_every_configuration():
    states = []
    for kw in (dict(), dict(degrees=30.0), dict(scale=(0.5, 2.0)), dict(shear=20.0), dict(flip=1.0), WILD):
        g = torch.Generator().manual_seed(11)
        draw_affine(3, 64, 6, generator=g, **kw)
        states.append(g.get_state())
    assert all(torch.equal(s, states[0]) for s in states[1:])
    g = torch.Generator().manual_seed(11)
    draw_crop_offsets(3, 6, g)
    assert not torch.equal(g.get_state(), states[0])                           # four more draws a clip than the crop's two


def test_inverse_times_forward_is_the_identity():
    g = torch.Generator().manual_seed(13)
    for _ in range(20):
        p = draw_affine_params(19, generator=g, **WILD)
        inv, fwd = affine_inverse(192, 19, *p), affine_forward(192, 19, *p)
        to3 = lambda m: torch.cat([m, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)])
        assert inv.dtype == torch.float64 and float((to3(inv) @ to3(fwd) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
        assert float((to3(fwd) @ to3(inv) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    # the composition: a point right of the centre goes down-right under a positive angle (y grows downwards), scaled
    fwd = affine_forward(65, 0, 0, 0, angle=90.0, scale=2.0)
    assert torch.allclose(fwd @ torch.tensor([33.0, 32.0, 1.0], dtype=torch.float64), torch.tensor([32.0, 34.0], dtype=torch.float64))
    sheared = affine_forward(65, 0, 0, 0, shear=45.0) @ torch.tensor([32.0, 33.0, 1.0], dtype=torch.float64)
    assert torch.allclose(sheared, torch.tensor([33.0, 33.0], dtype=torch.float64))
    # one rounding to fp32 of the float64 matrix
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert torch.equal(draw_affine(1, 192, 19, generator=g1, **WILD)[0],
                       affine_inverse(192, 19, *draw_affine_params(19, generator=g2, **WILD)).reshape(6).float())


def test_flip_probability_0_and_1():
    never = draw_affine(8, 64, 6, flip=0.0, generator=torch.Generator().manual_seed(1))
    always = draw_affine(8, 64, 6, flip=1.0, generator=torch.Generator().manual_seed(1))
    assert bool((never[:, 0] == 1).all()) and bool((always[:, 0] == -1).all())
    # the flip is about the centre, after RandomCrop's shift: x_src = (63 - x) - (left - pad) ... read back from the row
    assert torch.equal(always[:, 2], 63.0 - never[:, 2]) and torch.equal(always[:, [1, 3, 4, 5]], never[:, [1, 3, 4, 5]])
    half = draw_affine(64, 64, 6, flip=0.5, generator=torch.Generator().manual_seed(2))[:, 0]
    assert 0 < int((half < 0).sum()) < 64


# ------------------------------------------------------------------ the pipeline through the emulation
def _cfg(bs=2, **model):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "slowfast-LHand"
    cfg.MODEL.R3D_INPUT = KEY
    cfg.MODEL.DEPTH = 18
    cfg.NUM_CPU = 0
    for k, v in model.items():
        setattr(cfg.MODEL, k, v)
    return cfg


class Recording(EmuWarpBackend):
    """notes which of the three clip-writing launches RAN"""

    def __init__(self):
        super().__init__()
        self.launches = []

    def _noted(self, name, run):
        def wrapped(stream):
            self.launches.append(name)
            run(stream)
        return wrapped

    def u8_normalize_crop(self, *a, **kw):
        return self._noted("u8_normalize_crop", super().u8_normalize_crop(*a, **kw))

    def u8_pool_gather_crop(self, *a, **kw):
        return self._noted("u8_pool_gather_crop", super().u8_pool_gather_crop(*a, **kw))

    def u8_pool_gather_warp(self, *a, **kw):
        return self._noted("u8_pool_gather_warp", super().u8_pool_gather_warp(*a, **kw))


def test_config_defaults_and_affine_ranges():
    from video_classification_amd.config import get_cfg
    m = get_cfg().MODEL
    assert (m.AFFINE, m.AFFINE_DEGREES, tuple(m.AFFINE_SCALE), m.AFFINE_SHEAR, m.AFFINE_FLIP) == (False, 10.0, (0.85, 1.15), 0.0, 0.0)
    assert v1.affine_ranges(get_cfg()) is None
    assert v1.affine_ranges(_cfg(AFFINE=True, AFFINE_SHEAR=5.0)) == (10.0, (0.85, 1.15), 5.0, 0.0)


def test_device_preprocess_and_frame_pool_agree_stacked_against_pooled():
    be = EmuWarpBackend()
    s = 40
    video = _pool(7, s, s, seed=5)
    index = torch.tensor([[0, 3, 6], [5, -1, 2]], dtype=torch.int32)
    warp = draw_affine(2, s, s // 10, generator=torch.Generator().manual_seed(6), **WILD)
    ext = torch.cat([video, torch.full_like(video[:1], 127)])
    stacked = ext[torch.where(index < 0, torch.tensor(7), index.long())]        # (2, 3, s, s, 21), the missing frame as bytes of 127
    pool = FramePool("cpu", be)
    base = pool.add(video)
    rows = pool.rows(base, index)
    pre = DevicePreprocess("cpu", be)
    a, b = pre(stacked, warp=warp), pool.gather(rows, warp=warp)
    assert torch.equal(a, b) and torch.equal(a, R.warp32(video, index, LUT, 127, warp)) and a.abs().max() > 1
    assert torch.equal(pool.gather(rows, torch.float32, 5, 15, warp=warp), a[:, :, 5:20])
    first = pool._tables["warp"].data_ptr()
    pool.gather(rows, warp=identity_warp_rows(2))
    assert pool._tables["warp"].data_ptr() == first and pool._tables["warp"].dtype == torch.float32     # the address persists
    assert torch.equal(pre(stacked, warp=identity_warp_rows(2)), pre(stacked))
    with pytest.raises(ValueError, match="crop and warp together"):
        pre(stacked, torch.zeros(2, 2, dtype=torch.int32), warp=warp)
    with pytest.raises(ValueError, match="crop and warp together"):
        pool.gather(rows, crop=torch.zeros(2, 2, dtype=torch.int32), warp=warp)
    with pytest.raises(ValueError, match="not finite"):
        pre(stacked, warp=torch.full((2, 6), float("nan")))
    with pytest.raises(ValueError, match="not finite"):
        pool.gather(rows, warp=torch.full((2, 6), float("inf")))


def _resident(cfg, be, ds, **kw):
    return ResidentTrainSet(ds, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=200, **kw)


def _clip_frames(ds, v, indices):
    from video_classification_amd.input_pipeline import unpool_item
    return unpool_item(ds.video_item(v, indices))[0][KEY + "_u8"]


def test_resident_train_set_batches_are_warp32_of_the_plans_rows():
    cfg = _cfg(AFFINE=True, AFFINE_SHEAR=5.0, AFFINE_FLIP=0.5)
    be = Recording()
    ds = v1.SyntheticChalearn(cfg, "train", num_videos=6, seed=3, frames_per_video=(2, 9), as_uint8=True)
    r = _resident(cfg, be, ds, affine=v1.affine_ranges(cfg))
    plan, got = r.plan(0), list(r.epoch(0))
    assert len(plan) == len(got) == 3 and be.launches == ["u8_pool_gather_warp"] * 3
    for batch, (videos, indices, rows, jitter) in zip(got, plan):
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (2, 6) and jitter is None and sorted(batch) == [KEY, "label"]
        frames = torch.stack([_clip_frames(ds, v, indices[n].tolist()) for n, v in enumerate(videos)])
        assert torch.equal(batch[KEY], R.warp32(frames, None, LUT, 127, rows))
        assert not torch.equal(rows[:, [0, 1, 3, 4]], identity_warp_rows(2)[:, [0, 1, 3, 4]])
    with pytest.raises(ValueError, match="POOL_STEM.*AFFINE"):
        _resident(cfg, be, ds, affine=v1.affine_ranges(cfg), stem_channels=[(0, 5), (5, 15)])


def test_degenerate_affine_batches_are_the_crop_routes_clips():
    be = Recording()
    on = _cfg(AFFINE=True, AFFINE_DEGREES=0.0, AFFINE_SCALE=(1.0, 1.0))
    ds = v1.SyntheticChalearn(on, "train", num_videos=4, seed=3, frames_per_video=(2, 9), as_uint8=True)
    warped = list(_resident(on, be, ds, affine=v1.affine_ranges(on)).epoch(0))
    cropped = list(_resident(_cfg(), be, ds).epoch(0))
    assert be.launches == ["u8_pool_gather_warp"] * 2 + ["u8_pool_gather_crop"] * 2
    for a, b in zip(warped, cropped):
        assert torch.equal(a[KEY], b[KEY]) and torch.equal(a["label"], b["label"])


def test_with_affine_off_items_plans_and_launches_are_the_parents():
    cfg = _cfg()
    be = Recording()
    for kw in (dict(as_uint8=True), dict(raw=True)):
        ds = v1.SyntheticChalearn(cfg, "train", num_videos=3, seed=2, **kw)
        item = ds[1]
        g = torch.Generator().manual_seed(2 * 7919 + 1 * 31)
        torch.randint(0, 256, (4, 21, 64, 64), generator=g, dtype=torch.uint8)
        assert "warp" not in item and item["crop"].dtype == torch.int32 and torch.equal(item["crop"], draw_crop_offsets(1, 6, g)[0])
    ds = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=3, frames_per_video=(2, 9), as_uint8=True)
    r = _resident(cfg, be, ds)
    assert r.affine is None
    for videos, indices, crop, jitter in r.plan(0):
        assert crop.dtype == torch.int32 and tuple(crop.shape) == (2, 2) and jitter is None
        for n, v in enumerate(videos):
            g = r._clip_generator(0, v)
            torch.randint(0, max(0, r.seq_len(v) - 4) + 1, (1,), generator=g)
            assert torch.equal(crop[n], draw_crop_offsets(1, 6, g)[0])
    list(r.epoch(0))
    assert be.launches == ["u8_pool_gather_crop"] * 2
    # a train step of the Trainer, host fed: DevicePreprocess's sfk_u8_normalize_crop launch and nothing of the new header
    be.launches.clear()
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    t = v1.Trainer(cfg, train_set=ds, test_set=te, device="cpu", backend=be)
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append(sorted(batch)), prepare(batch))[1]
    assert math.isfinite(t.train_epoch()[0])
    assert be.launches == ["u8_normalize_crop"] * 2 and seen == [[KEY + "_u8", "crop", "label"]] * 2


@pytest.mark.parametrize("name", ["slowfast-LHand", "res3d", "res2d"])
def test_trainer_epoch_with_affine_on_issues_one_warp_launch_a_step(name):
    cfg = _cfg(AFFINE=True, COLOR_JITTER=True, RES2D_BACKEND="engine")
    cfg.MODEL.NAME = name
    be = Recording()
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    item = tr[0]
    assert sorted(item) == [KEY + "_u8", "jitter", "label", "warp"] and item["warp"].dtype == torch.float32 and tuple(item["warp"].shape) == (6,)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    seen = []
    prepare = t.mm.prepare_data

    def spy(batch):
        plain = prepare({k: v for k, v in batch.items() if k != "jitter"})[0]
        seen.append((batch, plain))
        return prepare(batch)
    t.mm.prepare_data = spy
    assert math.isfinite(t.train_epoch()[0])
    assert [k for k in be.launches if k != "u8_normalize_crop"] == ["u8_pool_gather_warp"] * 4 and "u8_normalize_crop" not in be.launches
    for batch, plain in seen:
        want = R.warp32(batch[KEY + "_u8"], None, LUT, 127, batch["warp"])
        x = plain if isinstance(plain, torch.Tensor) else torch.cat(list(plain), 1)
        c = x.shape[1] if name != "res2d" else x.shape[2]
        got = x.permute(0, 2, 1, 3, 4) if name != "res2d" else x
        assert torch.equal(got, want[:, :, :c])


def test_raw_and_video_items_carry_warp_under_affine():
    cfg = _cfg(AFFINE=True)
    item = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, raw=True)[0]
    assert "crop" not in item and tuple(item["warp"].shape) == (6,)
    assert "warp" not in v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=1, as_uint8=True)[0][0]
    labels = [("a/v0.avi", "d", 3)]
    frame = lambda path, size: torch.full((size, size, 21), 9, dtype=torch.uint8)
    ds = v1.ChalearnVideoFramesU8(cfg, "train", labels=labels, read_frame=frame)
    ds._video = lambda index: ("a/v0", ["0.jpg", "1.jpg"], 2)
    item = ds[0]
    assert sorted(item) == [KEY + "_u8", "label", "warp"] and item["warp"].dtype == torch.float32
    ds.cfg = _cfg()
    assert sorted(ds[0]) == [KEY + "_u8", "crop", "label"]


def test_refusals():
    be = EmuWarpBackend()
    warp, label = identity_warp_rows(2), torch.tensor([0, 1])
    frames = torch.zeros(2, 4, 64, 64, 21, dtype=torch.uint8)
    mm = v1.ModelManager(_cfg(U8_STEM=True), "cpu", be)
    with pytest.raises(ValueError, match="U8_STEM.*no float clip.*'warp'"):
        mm.prepare_data({KEY + "_u8": frames, "warp": warp, "label": label})
    pool = FramePool("cpu", be)
    rows = pool.rows(pool.add(frames[0]), torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=torch.int32))
    mm = v1.ModelManager(_cfg(POOL_STEM=True), "cpu", be)
    with pytest.raises(ValueError, match="POOL_STEM.*no float clip.*'warp'"):
        mm.prepare_data({KEY: pool.clip(rows, [(0, 5), (5, 15)]), "warp": warp, "label": label})
    for name in ("slowfast-LHand", "res3d", "res2d"):
        cfg = _cfg(RES2D_BACKEND="engine")
        cfg.MODEL.NAME = name
        with pytest.raises(ValueError, match="'warp' entry beside a float32 loader batch.*already cropped"):
            v1.ModelManager(cfg, "cpu", be).prepare_data({KEY: torch.zeros(2, 4, 21, 64, 64), "warp": warp, "label": label})
    with pytest.raises(ValueError, match="'warp' entry needs MODEL.RES2D_BACKEND = 'engine'"):
        cfg = _cfg(RES2D_BACKEND="torch")
        cfg.MODEL.NAME = "res2d"
        v1.ModelManager(cfg, "cpu", be).prepare_data({KEY: torch.zeros(2, 4, 21, 64, 64), "warp": warp, "label": label})


# ------------------------------------------------------------------ the ABI of include/sfk_warp.h, through the built library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from video_classification_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfk_warp.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_WARP) == ["sfk_u8_pool_gather_warp", "sfk_warp_abi_version", "sfk_warp_fallback_tiles"]
    for n in names:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_WARP[n]), n
    assert lib.sfk_warp_abi_version() == _lib.WARP_ABI_VERSION == 1
    assert callable(_lib.HipBackend.u8_pool_gather_warp) and callable(_lib.HipBackend.warp_fallback_tiles)
    assert "u8_pool_warp.hip" in open(os.path.join(ROOT, "video-classification_amd", "build.py")).read()
    # sfk_pool_crop_desc with warp in place of crop and pad
    crop = [f for f, _ in _lib._PoolCropDesc._fields_ if f not in ("crop", "pad")]
    assert [f for f, _ in _lib._PoolWarpDesc._fields_ if f != "warp"] == crop
    # include/sfk.h and the ABI lock are not touched by this header: none of its names is in them
    for other in ("sfk.h", "sfk.abi"):
        assert "warp" not in open(os.path.join(ROOT, "include", other)).read()


def test_struct_size_offsets_and_constants_match_the_header(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_warp.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(sfk_pool_warp_desc), '
                                  'offsetof(sfk_pool_warp_desc, index), offsetof(sfk_pool_warp_desc, lut), '
                                  'offsetof(sfk_pool_warp_desc, warp), offsetof(sfk_pool_warp_desc, fill), '
                                  'offsetof(sfk_pool_warp_desc, out), SFK_WARP_ABI_VERSION, SFK_WARP_TILE_H, SFK_WARP_TILE_W, '
                                  'SFK_WARP_LDS_BYTES, SFK_WARP_MAX_BLOCKS); return 0; }\n')
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib._PoolWarpDesc
    assert out[:6] == [ctypes.sizeof(D), D.index.offset, D.lut.offset, D.warp.offset, D.fill.offset, D.out.offset]
    assert out[0] == 104 == _lib.new_pool_warp_desc().struct_size
    assert out[6:] == [_lib.WARP_ABI_VERSION, _lib.WARP_TILE_H, _lib.WARP_TILE_W, _lib.WARP_LDS_BYTES, 1 << 23]
    assert (_lib.WARP_TILE_H, _lib.WARP_TILE_W) == (R.TILE_H, R.TILE_W)
    # the budget leaves at least two workgroups a CU their LDS (160 KiB a CU), the table's eight copies (8 KB) included
    assert 2 * (_lib.WARP_LDS_BYTES + 8 * 1024) <= 160 * 1024


def _good_desc(pool, index, lut, warp, out):
    from video_classification_amd import _lib
    d = _lib.new_pool_warp_desc()
    d.out_dtype, d.pool, d.index, d.lut, d.out = _lib.SFK_F32, pool.data_ptr(), index.data_ptr(), lut.data_ptr(), out.data_ptr()
    d.warp = warp.data_ptr()
    d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.fill = 3, 8, 8, 0, 5, 2, 2, 127
    d.frame_stride, d.row_stride, d.pixel_pitch = 8 * 8 * 5, 8 * 5, 5
    return d


def test_host_side_rejections_launch_nothing(lib):
    """every call here is refused before any launch (no GPU in this test): sfk_u8_pool_gather_crop's cases minus pad, plus a
    NULL warp; a NULL index is NOT one of them, so it is only shown to get past the argument checks to the size check"""
    pool = torch.zeros(3 * 8 * 8 * 5, dtype=torch.uint8)
    index, lut, warp = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(256), identity_warp_rows(2)
    out = torch.zeros(2 * 2 * 5 * 8 * 8 + 8)
    out = out[(-out.data_ptr() // 4) % 4:]                                    # 16-byte aligned
    assert out.data_ptr() % 16 == 0
    before = out.clone()
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 96), ("struct_size", 100), ("struct_size", 112), ("pool", None),
                         ("lut", None), ("warp", None), ("out", None), ("frames", 0), ("h", 0), ("w", -1), ("c", 0), ("n", 0),
                         ("t", -2), ("frame_stride", -1), ("row_stride", -40), ("c0", -1), ("pixel_pitch", 4), ("c0", 1),
                         ("fill", -1), ("fill", 256), ("out_dtype", 2), ("out_dtype", -1), ("out", out.data_ptr() + 4),
                         ("out", out.data_ptr() + 8)]:
        d = _good_desc(pool, index, lut, warp, out)
        setattr(d, field, value)
        assert lib.sfk_u8_pool_gather_warp(B(d), None) == -1, (field, value)
    assert lib.sfk_u8_pool_gather_warp(None, None) == -1
    for fields in [{"n": (1 << 23) + 1, "t": 1}, {"n": 1 << 12, "t": 1 << 12}, {"h": 16 * (1 << 22), "w": 33},
                   {"n": 2 ** 31 - 1, "t": 2 ** 31 - 1, "h": 2 ** 31 - 1, "w": 2 ** 31 - 1}]:
        for no_index in (False, True):
            d = _good_desc(pool, index, lut, warp, out)
            for k, v in fields.items():
                setattr(d, k, v)
            if no_index:
                d.index = None
            assert lib.sfk_u8_pool_gather_warp(B(d), None) == -2, (fields, no_index)
    assert torch.equal(out, before)
    # the host-side predicate
    m = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
    assert lib.sfk_warp_fallback_tiles(48, 40, 21, 21, m) == 0 and lib.sfk_warp_fallback_tiles(192, 192, 21, 21, m) == 0
    for args in [(0, 40, 21, 21, m), (48, 0, 21, 21, m), (48, 40, 21, 0, m), (48, 40, 20, 21, m), (48, 40, 21, 21, None)]:
        assert lib.sfk_warp_fallback_tiles(*args) == -1, args[:4]
    assert lib.sfk_warp_fallback_tiles(2 ** 31 - 1, 2 ** 31 - 1, 21, 21, m) == -2


def test_the_predicate_says_which_matrices_cannot_be_staged(lib):
    from video_classification_amd._lib import HipBackend
    hip = HipBackend.__new__(HipBackend)                                      # the binding without a device: the call is host only
    hip.lib = lib
    assert hip.warp_fallback_tiles(48, 40, 21, 21, R.MINIFY) > 0               # 3x minification of a frame larger than the budget
    assert hip.warp_fallback_tiles(24, 40, 21, 21, R.MINIFY) == 0              # the whole frame fits: nothing to fall back from
    assert hip.warp_fallback_tiles(48, 40, 21, 21, [float("nan")] * 6) == 6    # corners that are no numbers: every tile
    for row in R.FAR:
        assert hip.warp_fallback_tiles(48, 40, 21, 21, row) == 0               # no tap inside the frame: nothing is read at all
    # the config defaults at the production geometry stage every tile; the wild test ranges do not
    g = torch.Generator().manual_seed(0)
    mild = draw_affine(16, 192, 19, 10.0, (0.85, 1.15), generator=g)
    assert all(hip.warp_fallback_tiles(192, 192, 21, 21, r.tolist()) == 0 for r in mild)
    wild = draw_affine(16, 192, 19, generator=g, **WILD)
    assert any(hip.warp_fallback_tiles(192, 192, 21, 21, r.tolist()) > 0 for r in wild)


# ------------------------------------------------------------------ the mutants
def _emu_gather(be):
    def gather(pool, index, lut, fill, warp, c0, c, out_dtype):
        n, t = pool.shape[:2] if index is None else index.shape
        h, w = pool.shape[-3:-1]
        out = torch.empty(n, t, c, h, w, dtype=out_dtype)
        be.u8_pool_gather_warp(pool, index, lut, fill, warp, out, c0, c)(0)
        return out
    return gather


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_emulation_passes_the_checks_the_gpu_test_runs(out_dtype):
    R.check_all(_emu_gather(EmuWarpBackend()), out_dtype)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_refused_by_the_checks_the_gpu_test_runs(mutant):
    with pytest.raises(AssertionError, match="differ from warp32"):
        R.check_all(_emu_gather(EmuWarpBackend(mutant=mutant)))
