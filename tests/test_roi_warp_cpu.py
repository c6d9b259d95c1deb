"""include/sfk_roi_warp.h without a GPU: the references of tests/ref_roi_warp.py against the shipped resize reference, the
shared checks against the emulation and its six mutants, the ctypes binding against the header, the host-side rejections, and
the pipeline -- RoiResize(warp=), FramePool / BoxArena.roi_gather(warp=), ResidentGestureSet(affine=), the v2 datasets'
'warp' entry and a gesture_v2.Trainer epoch under MODEL.AFFINE -- on the emulation."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import ref_roi_warp as R
from emu_roi_warp import EmuRoiWarpBackend
from emu_v2 import roi_resize_ref
from video_classification_amd import _lib
from video_classification_amd import gesture_v2 as v2
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import (BoxArena, FramePool, ResidentGestureSet, RoiResize, byte_lut, draw_affine,
                                                     draw_crop_offsets)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfk_roi_warp.h")
H, W = 48, 64                                                  # the synthetic videos of the pipeline tests
WILD = (30.0, (0.6, 1.6), 10.0, 0.5)
DEGENERATE = (0.0, (1.0, 1.0), 0.0, 0.0)


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("antialias", [False, True], ids=["aa0", "aa1"])
def test_integer_translation_rows_of_roi_warp32_are_the_resize_then_the_crop(antialias):
    """within the 2e-6 tests/test_gpu_v2.py grants F.interpolate; the 'same' box has the extent of the output, where the
    integer resize takes its in == out shortcut and roi_warp32 the general formulas"""
    oh, ow = R.BOX_SIZE
    rows, tl, pad = R.crop_rows(oh, ow)
    assert (R.BOXES["same"][3] - R.BOXES["same"][1], R.BOXES["same"][2] - R.BOXES["same"][0]) == (oh, ow)
    for name, box in R.BOXES.items():
        src = R.random_clip(len(rows), 2, seed=1)
        bx = torch.tensor([box] * len(rows), dtype=torch.int32)
        got = R.roi_warp32(src, byte_lut(), bx, torch.tensor(rows), oh, ow, antialias)
        want = roi_resize_ref(src, byte_lut(), bx, oh, ow, antialias, torch.tensor(tl, dtype=torch.int32), pad)
        assert bool(want.any()) and float((got - want).abs().max()) <= 2e-6, name
        if name == "same":                                     # no interpolation at all: the bytes themselves
            assert torch.equal(got, want)


def test_roi_warp32_is_within_the_derived_bound_of_roi_warp64_and_non_finite_rows_give_zeros():
    for name, case in R.all_cases().items():
        a = R.expected32(case).double()
        b = R.roi_warp64(case["src"], byte_lut(), case["box"], case["warp"], case["out_h"], case["out_w"], case["antialias"])
        bd = R.bound(case["box"], case["src"].shape[2], case["src"].shape[3], case["out_h"], case["out_w"], case["antialias"], byte_lut())
        assert bool(b.any()) and float((a - b).abs().max()) <= bd < 1e-3, (name, float((a - b).abs().max()), bd)
    src = R.random_clip(3, 1, seed=2)
    bad = torch.tensor([[float("nan"), 0, 0, 0, 1, 0], [1, 0, float("inf"), 0, 1, 0], [1, 0, 0, 0, float("-inf"), 3]])
    out = R.roi_warp32(src, byte_lut(), torch.tensor([R.BOXES["down3"]] * 3, dtype=torch.int32), bad, 13, 18, True)
    assert not out.any() and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ the shared checks: the emulation passes, every mutant is refused
def test_the_emulation_passes_the_shared_checks():
    R.check_all(EmuRoiWarpBackend(), "cpu")
    for name in ("box_down3_aa1", "global_aa0"):
        R.check_f64(EmuRoiWarpBackend(), "cpu", name, R.all_cases()[name])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_is_refused_by_the_shared_checks(mutant):
    with pytest.raises(AssertionError):
        R.check_all(EmuRoiWarpBackend(mutant=mutant), "cpu", dtypes=(torch.float32,))


# ------------------------------------------------------------------ the binding against the header
def _header_structs():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", text, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            typ, names = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).groups()
            fields += [(n.strip().lstrip("*"), ("*" in typ or n.strip().startswith("*")) and "ptr" or typ.strip()) for n in names.split(",")]
        out[name] = fields
    return out


CTYPE = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "ptr": ctypes.c_void_p}


@pytest.mark.parametrize("cname,mirror", [("sfk_roi_warp_desc", _lib._RoiWarpDesc), ("sfk_roi_pool_warp_desc", _lib._RoiPoolWarpDesc),
                                          ("sfk_roi_ragged_warp_desc", _lib._RoiRaggedWarpDesc)])
def test_the_ctypes_mirrors_match_the_header_field_by_field(cname, mirror):
    fields = _header_structs()[cname]
    assert [n for n, _ in fields] == [n for n, _ in mirror._fields_]
    assert [CTYPE[t] for _, t in fields] == [t for _, t in mirror._fields_]
    text = open(HEADER).read()
    assert int(re.search(r"#define SFK_ROI_WARP_ABI_VERSION (\d+)", text).group(1)) == _lib.ROI_WARP_ABI_VERSION
    assert int(re.search(r"#define SFK_ROI_WARP_TILE_H (\d+)", text).group(1)) == _lib.ROI_WARP_TILE_H == R.TILE_H
    assert int(re.search(r"#define SFK_ROI_WARP_TILE_W (\d+)", text).group(1)) == _lib.ROI_WARP_TILE_W == R.TILE_W
    assert eval(re.search(r"#define SFK_ROI_WARP_LDS_BYTES (\(.*?\))", text).group(1)) == _lib.ROI_WARP_LDS_BYTES == R.STAGE_BYTES


def test_the_descriptor_sizes_are_what_gcc_says(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "sfk_roi_warp.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(sfk_roi_warp_desc), sizeof(sfk_roi_pool_warp_desc), sizeof(sfk_roi_ragged_warp_desc)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib._RoiWarpDesc), ctypes.sizeof(_lib._RoiPoolWarpDesc), ctypes.sizeof(_lib._RoiRaggedWarpDesc)]


@pytest.fixture(scope="module")
def lib():
    from video_classification_amd.build import build
    return ctypes.CDLL(build())


def test_the_library_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    assert lib.sfk_roi_warp_abi_version() == _lib.ROI_WARP_ABI_VERSION
    INVALID, UNSUPPORTED = -1, -2
    P = 0x1000                                                 # any non-NULL pointer: nothing is dereferenced on the host

    def stacked(**kw):
        d = _lib.new_roi_warp_desc()
        d.src = d.lut = d.box = d.warp = d.dst = P
        d.sn, d.st, d.sh, d.sw, d.sc = 10 ** 6, 10 ** 5, 400, 7, 1
        d.n, d.t, d.h, d.w, d.c, d.out_h, d.out_w = 2, 3, 40, 56, 7, 16, 32
        d.dst_dtype, d.dn, d.dt, d.dc, d.dh = 0, 10 ** 6, 10 ** 5, 1000, 32
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sfk_roi_resize_warp(ctypes.byref(d), None)

    def pool(**kw):
        d = _lib.new_roi_pool_warp_desc()
        d.pool = d.index = d.lut = d.box = d.warp = d.dst = P
        d.frame_stride, d.row_stride, d.pixel_pitch, d.frames = 10 ** 5, 400, 7, 5
        d.n, d.t, d.h, d.w, d.c0, d.c, d.out_h, d.out_w, d.fill = 2, 3, 40, 56, 0, 7, 16, 32, 93
        d.dst_dtype, d.dn, d.dt, d.dc, d.dh = 0, 10 ** 6, 10 ** 5, 1000, 32
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sfk_roi_resize_pool_warp(ctypes.byref(d), None)

    def ragged(**kw):
        d = _lib.new_roi_ragged_warp_desc()
        d.arena = d.offset = d.hw = d.lut = d.box = d.warp = d.dst = P
        d.arena_bytes, d.pixel_pitch, d.c0, d.c = 4096, 7, 0, 7
        d.n, d.t, d.max_h, d.max_w, d.out_h, d.out_w, d.fill = 2, 3, 40, 56, 16, 32, 93
        d.dst_dtype, d.dn, d.dt, d.dc, d.dh = 0, 10 ** 6, 10 ** 5, 1000, 32
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sfk_roi_resize_ragged_warp(ctypes.byref(d), None)

    for fn in (stacked, pool, ragged):
        assert fn(struct_size=8) == INVALID and fn(warp=None) == INVALID and fn(lut=None) == INVALID and fn(box=None) == INVALID
        assert fn(dst=None) == INVALID and fn(antialias=2) == INVALID and fn(c_off=-1) == INVALID and fn(dst_dtype=7) == INVALID
        assert fn(n=0) == INVALID and fn(out_w=0) == INVALID and fn(dh=-1) == INVALID
        assert fn(c=17) in (UNSUPPORTED, INVALID) and fn(out_h=4) == UNSUPPORTED          # c > SFK_ROI_MAX_C; 40 / 4 > SFK_ROI_MAX_RATIO
    assert stacked(src=None) == INVALID and stacked(sh=-1) == INVALID and stacked(c=17) == UNSUPPORTED and stacked(sw=5000) == UNSUPPORTED
    assert pool(pool=None) == INVALID and pool(index=None) == INVALID and pool(frames=0) == INVALID and pool(fill=256) == INVALID
    assert pool(pixel_pitch=6) == INVALID and pool(c0=-1) == INVALID and pool(pixel_pitch=5000) == UNSUPPORTED
    assert ragged(arena=None) == INVALID and ragged(offset=None) == INVALID and ragged(hw=None) == INVALID and ragged(fill=-1) == INVALID
    assert ragged(arena_bytes=4095) == INVALID and ragged(arena=P + 2) == INVALID and ragged(max_h=0) == INVALID


# ------------------------------------------------------------------ the pipeline on the emulation
def _cfg(bs=2, jitter=False, t=4, affine=None, size=32):
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
    if affine is not None:
        cfg.MODEL.AFFINE = True
        cfg.MODEL.AFFINE_DEGREES, cfg.MODEL.AFFINE_SCALE, cfg.MODEL.AFFINE_SHEAR, cfg.MODEL.AFFINE_FLIP = affine
    return cfg


def _synthetic(cfg, n=6, seed=3, **kw):
    return v2.SyntheticGesture(cfg, "train", num_videos=n, seed=seed, h=H, w=W, min_box=8, videos=True, **kw)


def test_roi_resize_and_the_two_gathers_refuse_crop_with_warp_and_bad_rows():
    be = EmuRoiWarpBackend()
    frames = torch.randint(0, 256, (1, 2, H, W, 7), dtype=torch.uint8)
    box = torch.tensor([[2, 3, 40, 30]], dtype=torch.int32)
    rr = RoiResize(16, "cpu", be)
    with pytest.raises(ValueError, match="crop and warp"):
        rr(frames, box, crop=torch.zeros(1, 2, dtype=torch.int32), warp=torch.zeros(1, 6))
    with pytest.raises(ValueError, match="not finite"):
        rr(frames, box, warp=torch.tensor([[1.0, 0, float("nan"), 0, 1, 0]]))
    with pytest.raises(ValueError, match=r"\(n, 6\)"):
        rr(frames, box, warp=torch.zeros(1, 5))
    pool = FramePool("cpu", be)
    base = pool.add(frames[0])
    with pytest.raises(ValueError, match="crop and warp"):
        pool.roi_gather(pool.rows(base, torch.arange(2)[None]), box, 16, crop=torch.zeros(1, 2, dtype=torch.int32), warp=torch.zeros(1, 6))
    arena = BoxArena(1 << 20, "cpu", be)
    ab = arena.add(frames[0])
    with pytest.raises(ValueError, match="crop and warp"):
        arena.roi_gather(arena.offsets(ab, torch.arange(2)[None]), torch.tensor([[H, W]]), box, 16,
                         crop=torch.zeros(1, 2, dtype=torch.int32), warp=torch.zeros(1, 6))
    assert be.log == []
    # and the three routes agree with roi_warp32 of the same clip
    warp = draw_affine(1, 16, 1, *WILD, generator=torch.Generator().manual_seed(0))
    want = R.roi_warp32(frames, byte_lut(), box, warp, 16, 16, True)
    a = rr(frames, box, warp=warp)
    b = pool.roi_gather(pool.rows(base, torch.arange(2)[None]), box, 16, warp=warp)
    c = arena.roi_gather(arena.offsets(ab, torch.arange(2)[None]), torch.tensor([[H, W]]), box, 16, warp=warp)
    assert bool(want.any()) and torch.equal(a, want) and torch.equal(b, want) and torch.equal(c, want)
    assert be.log == ["roi_resize_warp", "roi_resize_pool_warp", "roi_resize_ragged_warp"]


def test_degenerate_affine_ranges_yield_the_batches_of_augment_true():
    be = EmuRoiWarpBackend()
    cfg = _cfg()
    ds = _synthetic(cfg, n=5, seed=4, frames_per_video=(2, 9))
    kw = dict(batch_size=2, drop_last=False, seed=9, capacity_frames=200)
    aug = ResidentGestureSet(ds, cfg, "cpu", be, augment=True, **kw)
    aff = ResidentGestureSet(ds, cfg, "cpu", be, affine=DEGENERATE, **kw)
    pad = 32 // 10
    for pa, pb in zip(aug.plan(1), aff.plan(1)):
        assert pa[0] == pb[0] and torch.equal(pa[1], pb[1]) and torch.equal(pa[2], pb[2])
        top, left = pa[3][:, 0].float(), pa[3][:, 1].float()
        one, zero = torch.ones_like(top), torch.zeros_like(top)
        assert pb[3].dtype == torch.float32 and torch.equal(pb[3], torch.stack([one, zero, left - pad, zero, one, top - pad], 1))
    a, b = list(aug.epoch(1)), list(aff.epoch(1))
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert torch.equal(x["label"], y["label"]) and bool(x["clip_v2"].any())
        assert float((x["clip_v2"] - y["clip_v2"]).abs().max()) <= 2e-6      # the emulation of the sibling is F.interpolate itself
    assert "roi_resize_pool_warp" in be.log and "roi_resize_pool" in be.log


@pytest.mark.parametrize("room", ["ample", "none"])
def test_the_frame_store_the_box_store_and_the_loader_route_agree_bit_for_bit(room):
    be = EmuRoiWarpBackend()
    cfg = _cfg(jitter=True)
    ds = _synthetic(cfg, n=5, seed=4, frames_per_video=(2, 9))
    kw = dict(batch_size=2, drop_last=False, seed=9, jitter=(0.5, 0.3, 0.2, 0.1), affine=WILD)
    fr = ResidentGestureSet(ds, cfg, "cpu", be, capacity_frames=200 if room == "ample" else 9, **kw)
    frame = H * W * 7
    spill = 2 * (4 * frame + 16)
    bx = ResidentGestureSet(ds, cfg, "cpu", be, store="box", capacity_bytes=spill + (200 * frame if room == "ample" else 16), **kw)
    rr = RoiResize(32, "cpu", be, antialias=True)
    for e in range(2):
        plan = fr.plan(e)
        a, b = list(fr.epoch(e)), list(bx.epoch(e))
        assert len(a) == len(b) == len(plan) == 3
        for x, y, entry in zip(a, b, plan):
            assert sorted(x) == sorted(y) == ["clip_v2", "jitter", "label"]
            for k in x:
                assert torch.equal(x[k], y[k]), (e, k)
            videos, indices, box, warp = entry[0], entry[1], entry[2], entry[3]
            assert warp.dtype == torch.float32 and tuple(warp.shape) == (len(videos), 6)
            stacked = torch.stack([ds.video_item(v, indices[n].tolist())["frames_pool"] for n, v in enumerate(videos)])
            assert torch.equal(rr(stacked, box, warp=warp), x["clip_v2"]) and bool(x["clip_v2"].any())
    assert (bx.spilled_clips > 0) == (room == "none")
    assert "roi_resize_pool" not in be.log and "roi_resize_ragged" not in be.log and "roi_resize" not in be.log


def test_the_draw_order_leaves_the_generator_where_the_crop_draw_plus_four_rands_leave_it():
    be = EmuRoiWarpBackend()
    cfg = _cfg()
    ds = _synthetic(cfg, n=3, seed=4, frames_per_video=(6, 9))
    rs = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=1, seed=5, capacity_frames=100, affine=WILD)
    g, h = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    row = rs._clip_rows(g, 0, [0, 1, 2, 3])[1]
    crop = draw_crop_offsets(1, 32 // 10, h)[0]
    for _ in range(4):
        torch.rand(1, dtype=torch.float64, generator=h)
    assert torch.equal(g.get_state(), h.get_state()) and tuple(row.shape) == (6,) and row.dtype == torch.float32
    g2 = torch.Generator().manual_seed(77)
    assert torch.equal(row, draw_affine(1, 32, 3, *WILD, generator=g2)[0])
    assert crop.dtype == torch.int32


def _trainer(cfg, be, resident=False):
    cfg.MODEL.RESIDENT_TRAIN = resident
    cfg.MODEL.RESIDENT_GB = 80 * H * W * 7 / 2 ** 30
    tr = _synthetic(cfg, n=4, seed=1, frames_per_video=(3, 8))
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
    return v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)


@pytest.mark.parametrize("resident", [False, True], ids=["loader", "resident"])
def test_a_v2_trainer_epoch_runs_under_model_affine_and_issues_the_old_launches_without_it(resident):
    logs = {}
    for affine in (None, (10.0, (0.85, 1.15), 0.0, 0.0)):
        torch.manual_seed(0)
        be = EmuRoiWarpBackend()
        t = _trainer(_cfg(affine=affine, size=64), be, resident)
        if resident:
            assert t.resident.affine == (None if affine is None else (10.0, (0.85, 1.15), 0.0, 0.0))
            t.train_loader = None
        t.epoch = 1
        loss, _ = t.train_epoch()
        assert loss == loss
        logs[affine is not None] = list(be.log)
    old = "roi_resize_pool" if resident else "roi_resize"
    assert logs[False] == [old, old]                           # AFFINE off: exactly the launches of before, none of the new
    assert logs[True] == [old + "_warp"] * 2                   # on: the same count, each replaced by its sibling


def test_train_items_carry_warp_only_under_model_affine():
    for affine in (None, WILD):
        cfg = _cfg(affine=affine, jitter=True)
        for ds in (_synthetic(cfg, n=2), v2.SyntheticGesture(cfg, "train", num_videos=2, h=H, w=W, min_box=8)):
            item = ds[0]
            assert ("warp" in item) is (affine is not None) and "crop" not in item and "jitter" in item
            if affine is not None:
                assert item["warp"].dtype == torch.float32 and tuple(item["warp"].shape) == (6,)
        test_item = v2.SyntheticGesture(cfg, "test", num_videos=2, h=H, w=W, min_box=8)[0][0]
        assert "warp" not in test_item
    assert v1.draw_crop_or_warp(_cfg(affine=WILD), 32)[0] == "warp"


def test_the_float_batch_is_refused_under_model_affine_and_evaluated_as_before():
    be = EmuRoiWarpBackend()
    cfg = _cfg(affine=WILD, size=64)
    t = _trainer(cfg, be)
    fb = {"rgb": torch.rand(2, 4, 3, 64, 64), "uv": torch.rand(2, 4, 2, 64, 64), "flow": torch.rand(2, 4, 2, 64, 64),
          "label": torch.tensor([1, 2])}
    x, _ = t.mm.prepare_data(fb)                               # outside train_epoch (evaluation): unchanged
    assert x[0].shape[1] == 5 and x[1].shape[1] == 2
    with pytest.raises(ValueError, match="MODEL.AFFINE"):
        t.mm.prepare_data(dict(fb, warp=torch.zeros(2, 6)))
    t.train_loader = [fb]
    with pytest.raises(ValueError, match="MODEL.AFFINE"):
        t.train_epoch()
    assert t.mm.train_affine is False
