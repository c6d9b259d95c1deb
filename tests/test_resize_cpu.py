"""The raw transport on CPU (include/sfk_resize.h, input_pipeline.PadResize / collate_raw / FramePool.add_raw, tests/ref_resize.py,
tests/emu_resize.py): the ctypes binding of the new header and its host-side rejections, the integer definition against the real
cubic in float64, the identity at m == S, the raw item forms and their collation, PadResize's table validation, and the Trainer
on the emulated backend -- a train step and run_eval from raw items against the same frames resized by the reference and sent
as uint8 items."""
import ctypes
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import ref_resize
from emu_resize import EmuResizeBackend
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import (MISSING_BYTE, FramePool, PadResize, collate_raw, make_pooled_item,
                                                     make_raw_item, make_raw_pooled_item, pack_raw_frames, raw_offsets,
                                                     uniform_windows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w, S): up and down, odd padding, wide, identity, the two ends of crop_resize_dict, one pixel
SHAPES = [(5, 3, 8), (9, 16, 8), (37, 23, 16), (16, 16, 16), (100, 61, 64), (30, 200, 64), (240, 320, 192), (1, 1, 8), (2, 7, 8),
          (150, 149, 128), (64, 64, 192)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def _bytes(shape, seed, binary=False):
    g = torch.Generator().manual_seed(seed)
    if binary:
        return (torch.randint(0, 2, shape, generator=g) * 255).to(torch.uint8)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


# ------------------------------------------------------------------ the binding of include/sfk_resize.h
def test_resize_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_resize.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_RESIZE) == ["sfk_resize_abi_version", "sfk_u8_pad_resize_cubic"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG,
                  _lib.SIGNATURES_POOL):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_RESIZE[n]), n
    assert lib.sfk_resize_abi_version() == _lib.RESIZE_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_RESIZE_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.RESIZE_MAX_LDS_BYTES == 128 * 1024 and re.search(r"#define\s+SFK_RESIZE_MAX_LDS_BYTES\s+\(128 \* 1024\)", src)
    body = re.search(r"typedef struct \{(.*?)\} sfk_resize_desc;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._ResizeDesc._fields_] == fields


def test_resize_desc_and_lds_bytes_are_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    geoms = [(640, 21, 192), (666, 21, 192), (667, 21, 192), (1, 1, 1), (50, 21, 64), (37, 5, 13)]
    (tmp_path / "s.c").write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sfk_resize.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sfk_resize_desc), offsetof(sfk_resize_desc, hw), '
        'offsetof(sfk_resize_desc, max_side), offsetof(sfk_resize_desc, out_frame_stride));\n' +
        "".join(f'printf("%lld\\n", (long long)SFK_RESIZE_LDS_BYTES({m}, {c}, {s}));\n' for m, c, s in geoms) + 'return 0; }\n')
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib._ResizeDesc
    assert tuple(vals[:4]) == (ctypes.sizeof(D), D.hw.offset, D.max_side.offset, D.out_frame_stride.offset)
    assert vals[0] == 72 == _lib.new_resize_desc().struct_size
    assert vals[4:] == [_lib.resize_lds_bytes(*g) for g in geoms]
    # the limits admit size 192 with 21 channels from sources of up to 666 pixels a side (640 is what the issue asks for)
    assert vals[4] <= _lib.RESIZE_MAX_LDS_BYTES and vals[5] <= _lib.RESIZE_MAX_LDS_BYTES < vals[6]


def _good_resize(src, offset, hw, out):
    from video_classification_amd import _lib
    d = _lib.new_resize_desc()
    d.src, d.src_bytes, d.offset, d.hw, d.out = src.data_ptr(), src.numel(), offset.data_ptr(), hw.data_ptr(), out.data_ptr()
    d.frames, d.c, d.size, d.max_side, d.fill, d.out_frame_stride = 2, 5, 8, 9, 127, 8 * 8 * 5
    return d


def test_resize_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    src = torch.zeros(2 * 9 * 7 * 5, dtype=torch.uint8)
    offset, hw = torch.tensor([0, 315]), torch.tensor([[9, 7], [9, 7]], dtype=torch.int32)
    out = torch.full((2 * 8 * 8 * 5,), 9, dtype=torch.uint8)
    before = out.clone()
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 68), ("struct_size", 80), ("src", None), ("offset", None),
                         ("hw", None), ("out", None), ("frames", 0), ("frames", -1), ("c", 0), ("size", 0), ("size", -8),
                         ("max_side", 0), ("src_bytes", -1), ("out_frame_stride", 8 * 8 * 5 - 1), ("out_frame_stride", -320),
                         ("fill", -1), ("fill", 256)]:
        d = _good_resize(src, offset, hw, out)
        setattr(d, field, value)
        assert lib.sfk_u8_pad_resize_cubic(B(d), None) == -1, (field, value)
    assert lib.sfk_u8_pad_resize_cubic(None, None) == -1
    for fields in [{"frames": (1 << 23) // 8 + 1}, {"max_side": 667, "c": 21, "size": 192, "out_frame_stride": 192 * 192 * 21},
                   {"max_side": 4000}, {"size": 12000, "out_frame_stride": 12000 * 12000 * 5, "frames": 1}]:
        d = _good_resize(src, offset, hw, out)                                # 2^23 + 8 workgroups; more LDS than a workgroup gets
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.sfk_u8_pad_resize_cubic(B(d), None) == -2, fields
    assert torch.equal(out, before)


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("binary", [False, True], ids=["random", "0_255"])
def test_integer_definition_is_within_one_of_the_float64_cubic(binary):
    worst = 0
    for k, (h, w, s) in enumerate(SHAPES):
        assert ref_resize.floors_agree(h, w, s), (h, w, s)
        img = _bytes((h, w, 21), 100 + k, binary).numpy()
        got, want = ref_resize.pad_resize_int(img, s), ref_resize.pad_resize_f64(img, s)
        assert got.dtype == np.uint8 and got.shape == (s, s, 21)
        diff = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
        print(f"({h}, {w}) -> {s}: max |int - f64| {diff}")
        assert diff <= 1, (h, w, s, diff)
        worst = max(worst, diff)
    assert worst == 1                                                         # the bound is met, not merely respected


def test_m_equal_size_copies_the_padded_source():
    for h, w in [(16, 16), (16, 9), (7, 16), (1, 16), (16, 1)]:
        img = _bytes((h, w, 21), h * 17 + w).numpy()
        taps, q, s = ref_resize.axis_table(16, 16)
        assert q.tolist() == [[0, 2048, 0, 0]] * 16 and s.tolist() == list(range(16))
        got = ref_resize.pad_resize_int(img, 16)
        assert np.array_equal(got, ref_resize.pad_square(img))
        m, nx, ny = ref_resize.pad_geometry(h, w)
        assert np.array_equal(got[ny:ny + h, nx:nx + w], img) and int(got.astype(np.int64).sum()) == int(img.astype(np.int64).sum())


def test_overshoot_clamps_at_both_ends():
    img = _bytes((12, 9, 5), 5, binary=True).numpy()
    for s in (16, 13):
        r = ref_resize.pad_resize_int(img, s, unclamped=True)
        out = ref_resize.pad_resize_int(img, s)
        assert int(r.min()) < 0 and int(r.max()) > 255
        assert bool((out[r < 0] == 0).all()) and bool((out[r > 255] == 255).all())


# ------------------------------------------------------------------ the raw items and their collation
def _ragged(t, seed, c=21, lo=3, hi=20):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (int(torch.randint(lo, hi + 1, (1,), generator=g)), int(torch.randint(lo, hi + 1, (1,), generator=g)), c),
                          generator=g, dtype=torch.uint8) for _ in range(t)]


def test_collate_raw_round_trips_items():
    clips = [_ragged(3, 1), _ragged(3, 2), _ragged(3, 3)]
    clips[1][2] = None                                                        # a missing frame
    items = []
    for i, fr in enumerate(clips):
        it = make_raw_item("k", fr, i)
        it["crop"] = torch.tensor([i, 2 * i], dtype=torch.int32)
        items.append(it)
    assert items[1]["raw_hw"].tolist()[2] == [0, 0] and items[1]["raw_hw"].dtype == torch.int32
    b = collate_raw(items)
    assert sorted(b) == ["crop", "k_raw", "label", "raw_hw", "raw_offset"]
    assert b["k_raw"].dtype == torch.uint8 and b["k_raw"].dim() == 1 and b["k_raw"].numel() == sum(it["k_raw"].numel() for it in items)
    assert b["label"].tolist() == [0, 1, 2] and b["crop"].tolist() == [[0, 0], [1, 2], [2, 4]]
    assert tuple(b["raw_hw"].shape) == (3, 3, 2) and b["raw_offset"].dtype == torch.int64 and tuple(b["raw_offset"].shape) == (3, 3)
    assert torch.equal(b["raw_offset"], raw_offsets(b["raw_hw"], 21))          # end to end, in item order
    for i, fr in enumerate(clips):
        for t, f in enumerate(fr):
            h, w = b["raw_hw"][i, t].tolist()
            if f is None:
                assert (h, w) == (0, 0)
                continue
            o = int(b["raw_offset"][i, t])
            assert torch.equal(b["k_raw"][o:o + h * w * 21].reshape(h, w, 21), f)
    # items without a raw entry: default_collate
    plain = [{"k_u8": torch.zeros(2, 4, 4, 21, dtype=torch.uint8), "label": 1}, {"k_u8": torch.ones(2, 4, 4, 21, dtype=torch.uint8), "label": 0}]
    p = collate_raw(plain)
    assert sorted(p) == ["k_u8", "label"] and tuple(p["k_u8"].shape) == (2, 2, 4, 4, 21) and p["label"].tolist() == [1, 0]


def test_raw_pooled_item_keeps_existing_frames_and_marks_missing_ones():
    frames = _ragged(25, 7)
    missing, calls = {5, 14}, []

    def read(i):
        calls.append(i)
        return None if i in missing else frames[i]
    win = uniform_windows(25, 4)
    item = make_raw_pooled_item("CropLHand", win, 3, read)
    assert sorted(item) == ["CropLHand_rawpool", "label", "raw_hw", "windows"] and item["label"] == 3
    assert calls == list(range(24))                                           # once each, referenced frames only
    kept = [f for i, f in enumerate(frames[:24]) if i not in missing]
    assert item["raw_hw"].tolist() == [[f.shape[0], f.shape[1]] for f in kept] and item["raw_hw"].dtype == torch.int32
    assert torch.equal(item["CropLHand_rawpool"], torch.cat([f.reshape(-1) for f in kept]))
    same = make_pooled_item("CropLHand", win, 3, lambda i: None if i in missing else torch.zeros(4, 4, 21, dtype=torch.uint8))
    assert torch.equal(item["windows"], same["windows"]) and (item["windows"] == -1).sum() == 2
    with pytest.raises(ValueError):
        make_raw_pooled_item("CropLHand", win, 3, lambda i: None)
    raw, hw = pack_raw_frames([None, frames[0], None])
    assert hw.tolist() == [[0, 0], list(frames[0].shape[:2]), [0, 0]] and torch.equal(raw, frames[0].reshape(-1))


def test_pad_resize_validates_the_table_before_anything_is_uploaded():
    class Never(EmuResizeBackend):
        def u8_pad_resize_cubic(self, *a, **k):
            raise AssertionError("launched")
    pr = PadResize(8, "cpu", Never(), channels=5)
    raw = torch.zeros(2 * 6 * 4 * 5, dtype=torch.uint8)
    good_hw = torch.tensor([[6, 4], [6, 4]], dtype=torch.int32)
    for offset, hw in [([0, 121], good_hw),                                   # the second frame ends one byte past the buffer
                       ([-1, 120], good_hw), ([0, 120], [[6, 4], [6, 5]]), ([0, 120], [[-1, 4], [6, 4]]),
                       ([0, 120], [[6, 4], [6, -4]]), ([0], good_hw), ([0, 120], [[6, 4, 1], [6, 4, 1]])]:
        with pytest.raises(ValueError):
            pr(raw, torch.tensor(offset), torch.as_tensor(hw))
    with pytest.raises(ValueError, match="LDS"):                              # more than the kernel stages
        PadResize(192, "cpu", Never())(torch.zeros(800 * 21, dtype=torch.uint8), torch.tensor([0]), torch.tensor([[1, 800]]))
    assert pr.bytes_uploaded == 0
    ok = PadResize(8, "cpu", EmuResizeBackend(), channels=5)
    src = _bytes((240,), 3)
    got = ok(src, torch.tensor([0, 0, 120]), torch.tensor([[6, 4], [0, 0], [4, 6]]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 8, 8, 5) and ok.bytes_uploaded == 240
    assert np.array_equal(got[0].numpy(), ref_resize.pad_resize_int(src[:120].reshape(6, 4, 5).numpy(), 8))
    assert np.array_equal(got[2].numpy(), ref_resize.pad_resize_int(src[120:].reshape(4, 6, 5).numpy(), 8))
    assert bool((got[1] == MISSING_BYTE).all())


def test_frame_pool_add_raw_equals_add_of_the_resized_frames():
    be = EmuResizeBackend()
    frames = _ragged(11, 9, lo=5, hi=30)
    win = uniform_windows(11, 4)
    item = make_raw_pooled_item("k", win, 0, lambda i: None if i == 2 else frames[i])
    a, b = FramePool("cpu", be), FramePool("cpu", be)
    base = a.add_raw(item["k_rawpool"], item["raw_hw"], 16, item["windows"])
    kept = [f for i, f in enumerate(frames[:8]) if i != 2]
    resized = torch.stack([torch.from_numpy(ref_resize.pad_resize_int(f.numpy(), 16)) for f in kept])
    base_b = b.add(resized, item["windows"])
    assert base == base_b == 0 and a.live == b.live == {0: 7} and tuple(a.arena.shape[1:]) == (16, 16, 21)
    assert a.bytes_uploaded == item["k_rawpool"].numel() == sum(f.numel() for f in kept)
    assert torch.equal(a.gather(a.rows(base, item["windows"])), b.gather(b.rows(base_b, item["windows"])))
    bad = item["windows"].clone()
    bad[0, 0] = 7
    with pytest.raises(ValueError):
        FramePool("cpu", be).add_raw(item["k_rawpool"], item["raw_hw"], 16, bad)
    with pytest.raises(ValueError):
        FramePool("cpu", be).add_raw(item["k_rawpool"][:-1], item["raw_hw"], 16, item["windows"])


# ------------------------------------------------------------------ the Trainer on the emulated backend
def _cfg(bs, u8_stem=False, name="slowfast-LHand"):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.U8_STEM = u8_stem
    cfg.NUM_CPU = 0
    return cfg


def _resized_u8_item(item, size=64):
    """the uint8 item holding the reference-resized frames of a raw train item"""
    hw, raw, frames, at = item["raw_hw"].tolist(), item["CropLHand_raw"], [], 0
    for h, w in hw:
        if h == 0:
            frames.append(torch.full((size, size, 21), MISSING_BYTE, dtype=torch.uint8))
            continue
        frames.append(torch.from_numpy(ref_resize.pad_resize_int(raw[at:at + h * w * 21].reshape(h, w, 21).numpy(), size)))
        at += h * w * 21
    out = {k: v for k, v in item.items() if k not in ("CropLHand_raw", "raw_hw")}
    out["CropLHand_u8"] = torch.stack(frames)
    return out


class _Resized(torch.utils.data.Dataset):
    """a raw set as the uint8 (train) or pooled (test) items of its reference-resized frames"""

    def __init__(self, raw_set):
        self.s = raw_set

    def __len__(self):
        return len(self.s)

    def __getitem__(self, i):
        it = self.s[i]
        if "CropLHand_raw" in it:
            return _resized_u8_item(it)
        hw, raw, frames, at = it["raw_hw"].tolist(), it["CropLHand_rawpool"], [], 0
        for h, w in hw:
            frames.append(torch.from_numpy(ref_resize.pad_resize_int(raw[at:at + h * w * 21].reshape(h, w, 21).numpy(), 64)))
            at += h * w * 21
        return {"CropLHand_pool": torch.stack(frames), "windows": it["windows"], "label": it["label"]}


def _step_logits(t, batch):
    x, y = t.mm.prepare_data(batch)
    t.model.train()
    t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)
    eng = t.model.engine
    pl = eng._plan_for(eng.input_view(x[0]), x[1], t.model.slow_t_index, True)
    return x, pl.logits.clone(), float(t.step.loss[0])


@pytest.mark.parametrize("u8_stem", [False, True], ids=["float_clip", "u8_stem"])
def test_train_step_from_raw_items_equals_the_step_from_the_resized_u8_items(u8_stem):
    cfg = _cfg(2, u8_stem)
    raw_set = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=3, raw=True, raw_side=(20, 90))
    te = v1.SyntheticChalearn(cfg, "test", num_videos=1, seed=2, as_uint8=True)
    assert sorted(raw_set[0]) == ["CropLHand_raw", "crop", "label", "raw_hw"] and len(set(map(tuple, raw_set[0]["raw_hw"].tolist()))) > 1
    res = []
    for tr in (raw_set, _Resized(raw_set), _Resized(raw_set)):
        torch.manual_seed(0)
        t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuResizeBackend())
        batch = (getattr(tr, "collate_fn", None) or torch.utils.data.dataloader.default_collate)([tr[0], tr[1]])
        res.append(_step_logits(t, batch))
        if tr is raw_set:                                 # the loader the Trainer built collates the raw items itself
            assert t.train_loader.collate_fn is collate_raw and sorted(batch) == ["CropLHand_raw", "crop", "label", "raw_hw", "raw_offset"]
            assert sorted(next(iter(t.train_loader))) == sorted(batch)
    (xr, lr, lossr), (xa, la, lossa), (_, lb, _) = res
    for a, b in zip(xr, xa):                              # what the stems are given: the same bytes through the same path
        if u8_stem:
            assert torch.equal(a.frames, b.frames) and torch.equal(a.crop, b.crop) and (a.c0, a.c, a.pad) == (b.c0, b.c, b.pad)
        else:
            assert torch.equal(a, b)
    spread = float((la - lb).abs().max())                 # run to run, uint8 items
    err = float((lr - la).abs().max())
    print(f"raw train step: |logits - u8 items'| {err:.3e}, u8 run-to-run {spread:.3e}, loss {lossr:.6f} / {lossa:.6f}")
    assert err <= spread and np.isfinite(lossr)


def test_res3d_and_res2d_engine_prepare_data_take_raw_batches():
    for name, extra in (("res3d", {}), ("res2d", {"RES2D_BACKEND": "engine"})):
        cfg = _cfg(2, name=name)
        for k, v in extra.items():
            cfg.MODEL[k] = v
        raw_set = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=5, raw=True, raw_side=(30, 70))
        mm = v1.ModelManager(cfg, "cpu", EmuResizeBackend())
        xr, yr = mm.prepare_data(collate_raw([raw_set[0], raw_set[1]]))
        xa, ya = mm.prepare_data(torch.utils.data.dataloader.default_collate([_resized_u8_item(raw_set[0]), _resized_u8_item(raw_set[1])]))
        assert torch.equal(xr, xa) and torch.equal(yr, ya) and xr.dtype == torch.float32


@pytest.mark.parametrize("bs", [2, 5])
def test_run_eval_from_raw_pooled_items_equals_run_eval_from_pooled_items(bs):
    cfg = _cfg(bs)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=4, seed=2, raw=True, frames_per_video=(3, 14), raw_side=(20, 90))
    assert sorted(te[0]) == ["CropLHand_rawpool", "label", "raw_hw", "windows"] and sum(te.nclips) > bs
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuResizeBackend())
    pooled = torch.utils.data.DataLoader(_Resized(te), batch_size=bs, shuffle=False, collate_fn=lambda x: x)
    a, b = t.run_eval(pooled), t.run_eval(pooled)
    spread = float(np.abs(a["ps"] - b["ps"]).max())                           # run to run, pooled
    sent_pooled = t.frame_pool.bytes_uploaded
    got = t.run_eval()
    assert got["sv"] == a["sv"] == te.nclips and np.array_equal(got["t"], a["t"]) and got["acc"] == a["acc"]
    err = float(np.abs(got["ps"] - a["ps"]).max())
    print(f"raw pooled run_eval bs {bs}: |ps - pooled| {err:.3e}, pooled run-to-run {spread:.3e}")
    assert err <= spread
    raw_bytes = sum(te[i]["CropLHand_rawpool"].numel() for i in range(len(te)))
    assert t.frame_pool.bytes_uploaded == raw_bytes and not t.frame_pool.live
    assert sent_pooled == sum(te[i]["raw_hw"].shape[0] for i in range(len(te))) * 64 * 64 * 21


# ------------------------------------------------------------------ the flag off
def _crc(t):
    return zlib.crc32(t.contiguous().numpy().tobytes())


def test_synthetic_chalearn_without_raw_is_what_it_was():
    """raw=False: labels, clip counts and every draw of an item come from the documented seeds exactly as before -- seed for the
    labels and counts, seed*7919 + i*31 + j for clip j of video i (bytes, then crop), seed*104729 + 1 and seed*7919 + i*31 + 17
    for a pooled video -- recomputed here and compared by checksum with the items"""
    cfg = _cfg(2)
    seed, n = 4, 3
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 7, (n,), generator=g).tolist()
    nclips = torch.randint(1, 4, (n,), generator=g).tolist()
    for flag in ({}, {"raw": False}):
        tr = v1.SyntheticChalearn(cfg, "train", num_videos=n, seed=seed, as_uint8=True, **flag)
        te = v1.SyntheticChalearn(cfg, "test", num_videos=n, seed=seed, as_uint8=True, **flag)
        fl = v1.SyntheticChalearn(cfg, "train", num_videos=n, seed=seed, **flag)
        assert tr.labels == labels and tr.nclips == nclips and not hasattr(tr, "collate_fn")
        for i in range(n):
            gi = torch.Generator().manual_seed(seed * 7919 + i * 31)
            u8 = torch.randint(0, 256, (4, 21, 64, 64), generator=gi, dtype=torch.uint8)
            crop = torch.tensor([int(torch.randint(0, 13, (1,), generator=gi)), int(torch.randint(0, 13, (1,), generator=gi))], dtype=torch.int32)
            it = tr[i]
            assert sorted(it) == ["CropLHand_u8", "crop", "label"] and it["label"] == labels[i]
            assert _crc(it["CropLHand_u8"]) == _crc(u8.permute(0, 2, 3, 1)) and torch.equal(it["crop"], crop)
            assert _crc(fl[i]["CropLHand"]) == _crc((u8.float() / 255.0 - 0.45) / 0.225)
            assert len(te[i]) == nclips[i] and sorted(te[i][0]) == ["CropLHand_u8", "label"]
            for j in range(nclips[i]):
                gj = torch.Generator().manual_seed(seed * 7919 + i * 31 + j)
                assert _crc(te[i][j]["CropLHand_u8"]) == _crc(torch.randint(0, 256, (4, 21, 64, 64), generator=gj, dtype=torch.uint8).permute(0, 2, 3, 1))
        po = v1.SyntheticChalearn(cfg, "test", num_videos=n, seed=seed, pooled=True, frames_per_video=(3, 9), **flag)
        nframes = torch.randint(3, 10, (n,), generator=torch.Generator().manual_seed(seed * 104729 + 1)).tolist()
        assert po.nframes == nframes and po.labels == labels
        gp = torch.Generator().manual_seed(seed * 7919 + 1 * 31 + 17)
        frames = torch.randint(0, 256, (nframes[1], 64, 64, 21), generator=gp, dtype=torch.uint8)
        used = sorted(set(uniform_windows(nframes[1], 4).flatten().tolist()))
        assert _crc(po[1]["CropLHand_pool"]) == _crc(frames[used])
    # with the flag on, the labels, the clip counts and a train item's crop are still those draws
    rw = v1.SyntheticChalearn(cfg, "train", num_videos=n, seed=seed, raw=True)
    assert rw.labels == labels and rw.nclips == nclips and rw.collate_fn is collate_raw
    assert torch.equal(rw[1]["crop"], v1.SyntheticChalearn(cfg, "train", num_videos=n, seed=seed, as_uint8=True)[1]["crop"])
    assert torch.equal(rw[1]["CropLHand_raw"], rw[1]["CropLHand_raw"]) and not torch.equal(rw[1]["raw_hw"], rw[2]["raw_hw"])


# ------------------------------------------------------------------ the frames loader
def test_chalearn_video_frames_u8_with_device_resize(tmp_path):
    from test_pool_cpu import _tree
    cfg, labels, _, _ = _tree(tmp_path, [11, 3], missing={(0, 5)})
    calls = []

    def read_raw(path):
        calls.append(str(path))
        if not os.path.exists(path):
            return None
        k = int(os.path.basename(path)[:5]) // 5
        return np.full((10 + k, 20 - k, 21), k, dtype=np.uint8)
    ds = v1.ChalearnVideoFramesU8(cfg, "test", labels, read_raw, resize="device")
    assert ds.collate_fn is collate_raw
    it = ds[0]                                                                # 11 frames, T 4: windows at 0 and 4
    assert len(calls) == len(set(calls)) == 8 and sorted(it) == ["CropLHand_rawpool", "label", "raw_hw", "windows"]
    assert it["windows"].tolist() == [[0, 1, 2, 3], [4, -1, 5, 6]]            # frame 5 has no file
    assert it["raw_hw"].tolist() == [[10 + k, 20 - k] for k in (0, 1, 2, 3, 4, 6, 7)]
    assert it["CropLHand_rawpool"].numel() == sum((10 + k) * (20 - k) * 21 for k in (0, 1, 2, 3, 4, 6, 7))

    class Fixed:
        def randint(self, lo, hi):
            return 4
    tr = v1.ChalearnVideoFramesU8(cfg, "train", labels, read_raw, resize="device")
    tr.rng = Fixed()
    item = tr[0]
    assert sorted(item) == ["CropLHand_raw", "crop", "label", "raw_hw"] and item["label"] == 0
    assert item["raw_hw"].tolist() == [[14, 16], [0, 0], [16, 14], [17, 13]]   # frames 4, (5 missing), 6, 7
    assert item["CropLHand_raw"].numel() == (14 * 16 + 16 * 14 + 17 * 13) * 21
    # the default stays the host resize, with no collate of its own
    host = v1.ChalearnVideoFramesU8(cfg, "test", labels, lambda p, s: None)
    assert host.resize == "host" and not hasattr(host, "collate_fn")
    with pytest.raises(ValueError):
        v1.ChalearnVideoFramesU8(cfg, "test", labels, read_raw, resize="gpu")
    with pytest.raises(ValueError):
        v1.ChalearnVideoFramesU8(cfg, "test", labels, read_raw, pooled=False, resize="device")
    # and the raw sets feed run_eval
    t = v1.Trainer(cfg, train_set=v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True), test_set=ds, device="cpu",
                   backend=EmuResizeBackend())
    res = t.run_eval()
    assert res["sv"] == [2, 1] and res["ps"].shape == (3, 7)
    assert t.frame_pool.bytes_uploaded == sum(ds[i]["CropLHand_rawpool"].numel() for i in range(2))


def test_default_raw_reader_needs_cv2_and_says_so(tmp_path):
    try:
        import cv2  # noqa: F401
    except Exception:
        with pytest.raises(RuntimeError, match="cv2"):
            v1.cv2_read_frame_raw(tmp_path / "00000.jpg")
    else:
        assert v1.cv2_read_frame_raw(tmp_path / "00000.jpg") is None
