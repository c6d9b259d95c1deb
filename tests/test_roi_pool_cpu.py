"""The device-resident v2 train set on CPU (include/sfk_roi_pool.h, FramePool.roi_gather, input_pipeline.ResidentGestureSet,
MODEL.RESIDENT_TRAIN on gesture_v2.Trainer, tests/emu_roi_pool.py): the ctypes binding of the new header and its host-side
rejections, the sampling plan against ResidentTrainSet's starts and ChalearnGestureFrames.clip_box's boxes, the residency and
upload accounting with ample and with half capacity, and the v2 Trainer switch with what it still refuses."""
import ctypes
import os
import pickle
import re
import shutil
import subprocess

import pytest
import torch

from emu_roi_pool import EmuRoiPoolBackend, materialise
from emu_v2 import roi_resize_ref
from video_classification_amd import gesture_v2 as v2
from video_classification_amd.input_pipeline import (NO_BOX, FramePool, ResidentGestureSet, ResidentTrainSet, RoiResize,
                                                     byte_lut)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
FRAME = H * W * 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the binding of include/sfk_roi_pool.h
def test_roi_pool_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_roi_pool.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_ROI_POOL) == ["sfk_roi_pool_abi_version", "sfk_roi_resize_pool"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG,
                  _lib.SIGNATURES_POOL, _lib.SIGNATURES_RESIZE, _lib.SIGNATURES_RESIDENT):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_ROI_POOL[n]), n
    assert lib.sfk_roi_pool_abi_version() == _lib.ROI_POOL_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_ROI_POOL_ABI_VERSION\s+(\d+)", src).group(1))
    body = re.search(r"typedef struct \{(.*?)\} sfk_roi_pool_desc;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._RoiPoolDesc._fields_] == fields
    # sfk_roi_desc with its source addressing (src and the five strides) replaced by the pool's, plus index and fill
    roi = [f for f, _ in _lib._RoiDesc._fields_ if f not in ("src", "sn", "st", "sh", "sw", "sc", "reserved0")]
    pool = ("pool", "frame_stride", "row_stride", "pixel_pitch", "frames", "c0", "index", "fill")
    assert sorted(f for f in fields if f not in pool) == sorted(roi)


def test_roi_pool_desc_size_is_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    names = ("pool", "index", "crop", "fill", "dst", "dh", "c_off")
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_roi_pool.h"\n'
                                  'int main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(sfk_roi_pool_desc), '
                                  + ", ".join(f"offsetof(sfk_roi_pool_desc, {n})" for n in names) + "); return 0; }\n")
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib._RoiPoolDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in names]
    assert got[0] == 168 == _lib.new_roi_pool_desc().struct_size


def _good_desc(pool, index, lut, box, crop, out):
    from video_classification_amd import _lib
    d = _lib.new_roi_pool_desc()
    d.antialias, d.pool, d.index, d.lut, d.box, d.crop = 1, pool.data_ptr(), index.data_ptr(), lut.data_ptr(), box.data_ptr(), crop.data_ptr()
    d.frame_stride, d.row_stride, d.pixel_pitch = 240 * 320 * 7, 320 * 7, 7
    d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.pad, d.fill = 3, 240, 320, 0, 7, 1, 2, 19, 127
    d.out_h, d.out_w, d.dst_dtype, d.dst, d.c_off = 192, 192, _lib.SFK_F32, out.data_ptr(), 0
    d.dn, d.dt, d.dc, d.dh = 2 * 7 * 192 * 192, 7 * 192 * 192, 192 * 192, 192
    return d


def test_roi_pool_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test): what sfk_roi_resize rejects, with its codes, and
    what sfk_u8_pool_gather rejects of a pool"""
    pool = torch.zeros(64, dtype=torch.uint8)
    index, lut, box = torch.zeros(2, dtype=torch.int32), torch.zeros(256), torch.zeros(4, dtype=torch.int32)
    crop, out = torch.zeros(2, dtype=torch.int32), torch.full((8,), 3.0)
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 164), ("struct_size", 176), ("pool", None), ("index", None),
                         ("lut", None), ("box", None), ("dst", None), ("frames", 0), ("frames", -5), ("n", 0), ("t", -1),
                         ("h", 0), ("w", -3), ("c", 0), ("out_h", 0), ("out_w", -1), ("frame_stride", -1), ("row_stride", -2240),
                         ("c0", -1), ("c0", 1), ("pixel_pitch", 6), ("fill", -1), ("fill", 256), ("dn", -1), ("dh", -1),
                         ("antialias", 2), ("pad", -1), ("c_off", -1), ("dst_dtype", 7)]:
        d = _good_desc(pool, index, lut, box, crop, out)
        setattr(d, field, value)
        assert lib.sfk_roi_resize_pool(B(d), None) == -1, (field, value)
    assert lib.sfk_roi_resize_pool(None, None) == -1
    # SFK_ERR_UNSUPPORTED, as sfk_roi_resize: c > SFK_ROI_MAX_C, 240/29 and 320/39 > SFK_ROI_MAX_RATIO, a pixel pitch > 4096
    for fields in [{"c": 17, "pixel_pitch": 17}, {"out_h": 29}, {"out_w": 39}, {"pixel_pitch": 4097},
                   {"out_h": 29, "crop": None}]:
        d = _good_desc(pool, index, lut, box, crop, out)
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.sfk_roi_resize_pool(B(d), None) == -2, fields
    # (the LDS fit cannot fail inside those bounds: the largest tile, 16 channels reduced 8x on both axes, needs 65 072 of the
    # 65 536 bytes, so there is no descriptor that reaches that rejection alone -- in either entry point)
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------ FramePool.roi_gather on the emulated backend
def test_roi_gather_is_roi_resize_of_the_materialised_clips_and_checks_liveness():
    be = EmuRoiPoolBackend()
    g = torch.Generator().manual_seed(3)
    a, b = (torch.randint(0, 256, (f, H, W, 7), generator=g, dtype=torch.uint8) for f in (4, 3))
    pool = FramePool("cpu", be)
    base_a, base_b = pool.add(a), pool.add(b)
    idx = torch.tensor([[0, 1, 2, 3], [6, -1, 4, 4], [3, 2, 2, 0]], dtype=torch.int32)
    box = torch.tensor([[3, 2, 40, 30], [0, 0, W, H], [-9, 20, 500, 33]], dtype=torch.int32)
    clips = materialise(pool.arena, idx, 127)
    assert torch.equal(clips[1, 1], torch.full((H, W, 7), 127, dtype=torch.uint8)) and torch.equal(clips[1, 0], b[2])
    for aa in (True, False):
        want = RoiResize(32, "cpu", be, antialias=aa)(clips, box)
        assert torch.equal(pool.roi_gather(idx, box, 32, torch.float32, aa), want)
        assert torch.equal(want, roi_resize_ref(clips, byte_lut(), box, 32, 32, aa))
    crop = torch.tensor([[0, 6], [3, 3], [6, 0]], dtype=torch.int32)
    want = RoiResize(32, "cpu", be)(clips, box, crop)
    assert torch.equal(pool.roi_gather(idx, box, 32, crop=crop), want) and not torch.equal(want, RoiResize(32, "cpu", be)(clips, box))
    out = torch.full((3, 4, 7, 32, 32), -7.0)
    assert pool.roi_gather(idx, box, 32, crop=crop, padding=3, out=out) is out and torch.equal(out, want)
    assert pool.roi_gather(idx, box, 32, torch.bfloat16).dtype == torch.bfloat16
    pool.release(base_a)
    with pytest.raises(ValueError, match="roi_gather"):                       # slots 0..3 are no longer a live video's
        pool.roi_gather(idx, box, 32)
    with pytest.raises(ValueError, match="roi_gather"):
        pool.roi_gather(torch.tensor([[7]], dtype=torch.int32), box[:1], 32)
    with pytest.raises(ValueError, match="roi_gather"):
        pool.roi_gather(torch.tensor([[-2]], dtype=torch.int32), box[:1], 32)
    assert tuple(pool.roi_gather(idx[1:2], box[1:2], 16).shape) == (1, 4, 7, 16, 16)


# ------------------------------------------------------------------ ResidentGestureSet: the plan
def _cfg(bs=2, root="/nonexistent", jitter=False, t=4):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = t
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "gesture-v2"
    cfg.MODEL.INPUT_SIZE = 64
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


def _synthetic(cfg, n=6, seed=3, **kw):
    return v2.SyntheticGesture(cfg, "train", num_videos=n, seed=seed, h=H, w=W, min_box=8, videos=True, **kw)


class Counting:
    """a train set seen through the four methods only, counting the calls"""

    def __init__(self, ds):
        self.ds, self.calls = ds, []

    def __len__(self):
        return len(self.ds)

    def seq_len(self, i):
        self.calls.append(("seq_len", i))
        return self.ds.seq_len(i)

    def label(self, i):
        self.calls.append(("label", i))
        return self.ds.label(i)

    def frame_boxes(self, i):
        self.calls.append(("frame_boxes", i))
        return self.ds.frame_boxes(i)

    def video_item(self, i, indices=None):
        self.calls.append(("video_item", i, None if indices is None else tuple(indices)))
        return self.ds.video_item(i, indices)


class Lengths:
    """a v1 train set of which only the frame counts matter"""

    def __init__(self, lengths):
        self.lengths = list(lengths)

    def __len__(self):
        return len(self.lengths)

    def seq_len(self, i):
        return self.lengths[i]

    def label(self, i):
        return 0

    def video_item(self, i, indices=None):
        raise AssertionError("the plan reads no frame")


def test_default_synthetic_gesture_is_unchanged_and_offers_nothing():
    cfg = _cfg()
    plain = v2.SyntheticGesture(cfg, "train", num_videos=4, seed=1, h=H, w=W, min_box=8)
    vids = v2.SyntheticGesture(cfg, "train", num_videos=4, seed=1, h=H, w=W, min_box=8, videos=True)
    assert (plain.labels, plain.nclips) == (vids.labels, vids.nclips)         # the default draws are not disturbed
    for m in ("seq_len", "label", "video_item", "frame_boxes"):
        assert not hasattr(plain, m) and callable(getattr(vids, m))
    assert sorted(plain[0]) == ["box", "frames_u8", "label"] and tuple(plain[0]["frames_u8"].shape) == (4, H, W, 7)
    item = vids[1]                                                            # the loader path: a random clip of the video
    assert sorted(item) == ["box", "frames_u8", "label"] and tuple(item["frames_u8"].shape) == (4, H, W, 7)
    fb = vids.frame_boxes(0)
    assert tuple(fb.shape) == (vids.seq_len(0), 4) and fb.dtype == torch.int32
    assert fb[5].tolist() == list(NO_BOX) and fb[0].tolist() != list(NO_BOX)
    it = vids.video_item(2, [3, 0])
    assert sorted(it) == ["frames_pool", "windows"] and it["windows"].tolist() == [[0, 1]]
    assert torch.equal(it["frames_pool"][1], vids.video_item(2)["frames_pool"][0])
    with pytest.raises(ValueError, match="frame_boxes"):
        ResidentGestureSet(plain, cfg, "cpu", EmuRoiPoolBackend(), batch_size=2, capacity_frames=99)


def test_plan_is_a_function_of_seed_and_epoch_and_its_starts_are_v1s():
    be = EmuRoiPoolBackend()
    cfg = _cfg(jitter=True)
    ds = _synthetic(cfg, frames_per_video=(2, 9))
    assert min(ds.vframes) <= 4 < max(ds.vframes)                             # a short video wraps
    jit = (0.5, 0.3, 0.2, 0.1)
    a = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=200, jitter=jit)
    b = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=9, jitter=jit)
    v1cfg = _cfg()
    v1cfg.MODEL.R3D_INPUT = "CropLHand"
    one = ResidentTrainSet(Lengths(ds.vframes), v1cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=99)
    aug = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=99, augment=True)
    for e in range(3):
        pa, pb, p1, pg = a.plan(e), b.plan(e), one.plan(e), aug.plan(e)
        assert len(pa) == len(pb) == len(p1) == 3 and sorted(v for entry in pa for v in entry[0]) == list(range(6))
        for (va, ia, ba, ca, ja), (vb, ib, bb, cb, jb), (v1, i1, c1, j1), (vg, ig, bg, cg, jg) in zip(pa, pb, p1, pg):
            assert va == vb == v1 == vg and torch.equal(ia, ib) and torch.equal(ia, i1) and torch.equal(ia, ig)   # v1's starts
            assert torch.equal(ba, bb) and torch.equal(ba, bg) and ca is None and cb is None and torch.equal(ja, jb)
            assert ia.dtype == torch.int32 and tuple(ia.shape) == (2, 4) and ba.dtype == torch.int32 and tuple(ba.shape) == (2, 4)
            assert tuple(ja.shape) == (2, 8) and j1 is None and jg is None
            assert torch.equal(cg, c1) and int(cg.min()) >= 0 and int(cg.max()) <= 12          # augment: v1's crop draw, S // 10 = 6
            for v, row in zip(va, ia.tolist()):
                n = ds.seq_len(v)
                assert 0 <= row[0] <= max(0, n - 4) and row == [(row[0] + k) % n for k in range(4)]
    assert [e[0] for e in a.plan(0)] != [e[0] for e in a.plan(1)] or not torch.equal(a.plan(0)[0][1], a.plan(1)[0][1])
    assert len(ResidentGestureSet(ds, cfg, "cpu", be, batch_size=4, capacity_frames=99).plan(0)[-1][0]) == 2   # drop_last=False


def _part_boxes(box, parts=(4, 19, 21)):
    """one frame's [25][4] DensePose part table with `box` split over the parts (None: the part is not there)"""
    pb = [None] * 25
    if box is not None:
        x1, y1, x2, y2 = box
        pb[parts[0]] = [x1, y1, (x1 + x2) // 2, y2]
        pb[parts[2]] = [(x1 + x2) // 2, (y1 + y2) // 2, x2, y2]
    return pb


def _write_videos(root, cfg, tables):
    """the box pickles of ChalearnGestureFrames under root, one video per table ([frame] -> box | None | 'noframe'); the
    pickle holds one entry more than the video has frames, as the reference's"""
    labels = []
    for i, rows in enumerate(tables):
        rel = f"train/{i:03d}/M_{i:05d}"
        p = root / cfg.CHALEARN.BOX / (rel + ".pkl")
        p.parent.mkdir(parents=True)
        with p.open("wb") as f:
            pickle.dump([None if r == "noframe" else _part_boxes(r) for r in rows] + [_part_boxes((1, 1, 5, 5))], f)
        labels.append((rel + ".avi", rel + ".avi", i + 2))
    return labels


def _read_video(path, channels, indices, fmt):
    """(T, C, H, W) uint8 whose bytes tell the video, the plane and the frame"""
    c = 3 if fmt == "rgb24" else channels
    vid = int(os.path.basename(str(path)).split("_")[-1][:5])
    base = {"1_Sample": 0, "5_UV_Video": 100, "2_Flow_New": 200}[[p for p in path.parts if p[:2] in ("1_", "5_", "2_")][-1]]
    out = torch.empty(len(indices), c, H, W, dtype=torch.uint8)
    for k, i in enumerate(indices):
        for ch in range(c):
            out[k, ch] = (base + 10 * vid + ch + 7 * i) % 256
    return out


TABLES = [
    [(5, 6, 30, 20), None, (2, 9, 50, 40), "noframe", (8, 8, 20, 20), (10, 3, 33, 44), None, (1, 1, 9, 9)],     # sentinels inside
    [(-7, -3, 30, 20), (40, 30, 90, 70), (10, 10, 70, 50), (3, 3, 64, 48), (0, 0, 65, 49), (50, 40, 100, 100)],  # beyond the frame
    [(5, 5, 20, 20), None, (30, 10, 60, 40)],                                 # seq_len 3 <= clip_len 4: the clip wraps
    [None, (12, 14, 40, 30), None, None, None, None, (2, 2, 8, 8)],           # clips with a single boxed frame
    [(0, 0, 64, 48)],                                                         # one frame
]


def test_boxes_equal_clip_box_and_chalearn_gesture_frames_offers_the_contract(tmp_path):
    cfg = _cfg(root=tmp_path)
    parts = v2.parts_of("lHandLoArm")
    assert parts == [4, 19, 21]
    ds = v2.ChalearnGestureFrames(cfg, "train", parts, "random", _write_videos(tmp_path, cfg, TABLES), read_video=_read_video)
    assert [ds.seq_len(i) for i in range(5)] == [8, 6, 3, 7, 1] and [ds.label(i) for i in range(5)] == [1, 2, 3, 4, 5]
    fb = ds.frame_boxes(0)
    assert fb.dtype == torch.int32 and tuple(fb.shape) == (8, 4)
    assert fb[0].tolist() == [5, 6, 30, 20] and fb[1].tolist() == list(NO_BOX) == fb[3].tolist()
    assert ds.frame_boxes(1)[0].tolist() == [-7, -3, 30, 20]                  # not clamped: the clip's union is
    it = ds.video_item(1, [4, 0, 4])
    assert sorted(it) == ["frames_pool", "windows"] and it["windows"].tolist() == [[0, 1, 2]]
    assert tuple(it["frames_pool"].shape) == (3, H, W, 7) and it["frames_pool"].dtype == torch.uint8
    assert it["frames_pool"][:, 0, 0].tolist() == [[(b + 10 + ch + 28) % 256 for b, ch in
                                                    ((0, 0), (0, 1), (0, 2), (100, 0), (100, 1), (200, 0), (200, 1))],
                                                   [10, 11, 12, 110, 111, 210, 211]] + [[38, 39, 40, 138, 139, 238, 239]]
    assert tuple(ds.video_item(2)["frames_pool"].shape) == (3, H, W, 7)
    # the loader item of the same video is those frames with clip_box's box: the two paths read the same bytes
    item = ds[4]
    assert torch.equal(item["frames_u8"], ds.video_item(4, [0, 0, 0, 0])["frames_pool"]) and item["box"].tolist() == [0, 0, 64, 48]
    seen = Counting(ds)
    r = ResidentGestureSet(seen, cfg, "cpu", EmuRoiPoolBackend(), batch_size=2, drop_last=False, seed=2, capacity_frames=60)
    assert r.frame_shape == (H, W, 7)
    raw = [pickle.load((tmp_path / cfg.CHALEARN.BOX / f"train/{i:03d}/M_{i:05d}.pkl").open("rb")) for i in range(5)]
    kinds = set()
    for e in range(12):
        for videos, indices, box, crop, jitter in r.plan(e):
            assert crop is None and jitter is None
            for n, v in enumerate(videos):
                idx = indices[n].tolist()
                assert torch.equal(box[n], ds.clip_box(raw[v], idx, H, W)), (e, v, idx)
                rows = ds.frame_boxes(v)[idx]
                kinds |= {"sentinel"} if (rows == torch.tensor(NO_BOX)).all(1).any() else set()
                kinds |= {"beyond"} if int(rows[:, 2].max()) > W or 0 > int(rows[:, 0].min()) > -100 else set()
                kinds |= {"wrap"} if len(set(idx)) < 4 else set()
    assert kinds == {"sentinel", "beyond", "wrap"}
    assert sorted(c for c in seen.calls if c[0] == "frame_boxes") == [("frame_boxes", i) for i in range(5)]   # once per video
    assert [c for c in seen.calls if c[0] == "video_item"] == [("video_item", 0, (0,))]    # the frame shape: one frame, once


def test_an_all_sentinel_clip_is_a_value_error_naming_the_video_at_plan_time(tmp_path):
    cfg = _cfg(root=tmp_path)
    tables = [[(5, 6, 30, 20)] * 5, [None, "noframe", None, None]]           # video 1: no part box in any frame
    ds = v2.ChalearnGestureFrames(cfg, "train", [4, 19, 21], "random", _write_videos(tmp_path, cfg, tables), read_video=_read_video)
    r = ResidentGestureSet(ds, cfg, "cpu", EmuRoiPoolBackend(), batch_size=2, capacity_frames=60)
    with pytest.raises(ValueError, match="video 1"):
        r.plan(0)
    assert r.bytes_uploaded == 0
    empty = [[(70, 5, 90, 20)] * 5]                                           # a box wholly right of the 64-pixel frame
    ds = v2.ChalearnGestureFrames(cfg, "train", [4, 19, 21], "random", _write_videos(tmp_path / "b", _cfg(root=tmp_path / "b"), empty),
                                  read_video=_read_video)
    ds.root = str(tmp_path / "b")
    with pytest.raises(ValueError, match="video 0.*empty"):
        ResidentGestureSet(ds, cfg, "cpu", EmuRoiPoolBackend(), batch_size=1, capacity_frames=60).plan(0)


# ------------------------------------------------------------------ ResidentGestureSet: residency, spill, the replay
def _replay(r, ds, be, epochs, on_batch=None):
    """every clip epoch(e) yields is RoiResize of video_item's frames at plan(e)'s indices with plan(e)'s box and crop"""
    roi = RoiResize(r.size, "cpu", be, out_dtype=r.out_dtype, antialias=r.antialias)
    for e in epochs:
        plan = r.plan(e)
        got = []
        for batch in r.epoch(e):
            if on_batch is not None:
                on_batch()
            got.append(batch)
        assert len(got) == len(plan)
        for batch, (videos, indices, box, crop, jitter) in zip(got, plan):
            assert sorted(batch) == sorted(["clip_v2", "label"] + (["jitter"] if jitter is not None else []))
            assert batch["label"].tolist() == [ds.label(v) for v in videos] and batch["label"].dtype == torch.int64
            if jitter is not None:
                assert torch.equal(batch["jitter"], jitter) and tuple(jitter.shape) == (len(videos), 8)
            frames = torch.stack([ds.video_item(v, indices[n].tolist())["frames_pool"] for n, v in enumerate(videos)])
            assert batch["clip_v2"].dtype == r.out_dtype and tuple(batch["clip_v2"].shape) == (len(videos), 4, 7, r.size, r.size)
            assert torch.equal(batch["clip_v2"], roi(frames, box, crop))


@pytest.mark.parametrize("augment", [False, True])
def test_resident_gesture_set_replays_its_plan_and_uploads_every_frame_once(augment):
    be = EmuRoiPoolBackend()
    cfg = _cfg(jitter=True)
    cfg.MODEL.RESIZE_ANTIALIAS = not augment
    ds = _synthetic(cfg, frames_per_video=(2, 9))
    seen = Counting(ds)
    r = ResidentGestureSet(seen, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=200,
                           jitter=(0.5, 0.3, 0.2, 0.1), augment=augment)
    assert (r.capacity, r.spill_slots, r.resident_slots, r.antialias) == (200, 8, 192, not augment)
    whole = sum(ds.vframes) * FRAME
    ptr = []
    _replay(r, seen, be, [0], on_batch=lambda: ptr.append(r.pool.arena.data_ptr()))
    assert r.bytes_uploaded == whole and r.resident_videos == 6 and r.resident_frames == sum(ds.vframes)
    assert r.spilled_clips == 0 and r.spill_peak == 0 and tuple(r.pool.arena.shape) == (200, H, W, 7)
    del seen.calls[:]
    for e in (1, 2):
        got = list(r.epoch(e))                                                # nothing to read: label is the only method called
        assert len(got) == 3 and {c[0] for c in seen.calls} == {"label"}
    assert r.bytes_uploaded == whole
    _replay(r, seen, be, [1, 2], on_batch=lambda: ptr.append(r.pool.arena.data_ptr()))
    assert r.bytes_uploaded == whole and len(set(ptr)) == 1
    assert not any(c[0] == "video_item" and c[2] is None for c in seen.calls)  # (the replay itself asks for the clips' frames)


def test_resident_gesture_set_with_half_the_capacity_spills_the_rest():
    be = EmuRoiPoolBackend()
    cfg = _cfg()
    ds = _synthetic(cfg, n=8, seed=4, frames_per_video=(2, 12))
    assert min(ds.vframes) <= 4                                               # a video no longer than a clip
    cap = sum(ds.vframes) // 2 + 2 * 4                                        # about half the frames, plus the spill region

    def run():
        seen = Counting(ds)
        r = ResidentGestureSet(seen, cfg, "cpu", be, batch_size=2, drop_last=False, seed=1, capacity_frames=cap)
        assert (r.resident_slots, r.spill_slots) == (cap - 8, 8)
        log = []
        for e in range(3):
            before = r.bytes_uploaded

            def check():
                assert sum(r.pool.live.values()) <= cap and r.spill_peak <= 8
            _replay(r, seen, be, [e], on_batch=check)
            resident = sorted(v for v, ok in r._resident.items() if ok)
            log.append((resident, r.bytes_uploaded - before, r.spilled_clips, dict(r.pool.live)))
            assert sorted(r.pool.live.values()) == sorted(ds.vframes[v] for v in resident)                    # spills released
        return r, log

    (r, log), (_, again) = run(), run()
    assert log == again                                                       # the same videos resident, the same uploads
    resident = log[0][0]
    assert 0 < len(resident) < 8 and log[1][0] == log[2][0] == resident and r.resident_videos == len(resident)
    assert sum(ds.vframes[v] for v in resident) == r.resident_used == r.resident_frames <= r.resident_slots
    used, want = 0, []                                                        # the rule, replayed: first come, first resident
    for entry in r.plan(0):
        for v in entry[0]:
            if used + ds.vframes[v] <= cap - 8:
                used += ds.vframes[v]
                want.append(v)
    assert sorted(want) == resident
    for e in (1, 2):                                                          # exactly the distinct frames of the spilled clips
        spilled = [(v, sorted(set(row.tolist()))) for entry in r.plan(e) for v, row in zip(entry[0], entry[1]) if v not in resident]
        assert log[e][1] == sum(len(ks) for _, ks in spilled) * FRAME > 0 and log[e][2] == len(spilled) == 8 - len(resident)
    assert 0 < r.spill_peak <= 8
    with pytest.raises(ValueError, match="no resident slot"):
        ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, capacity_frames=8)
    cfg.MODEL.RESIDENT_GB = 20 * FRAME / 2 ** 30                              # the default capacity: floor(GB * 2^30 / (H*W*7))
    assert ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2).capacity == 20


# ------------------------------------------------------------------ the v2 Trainer switch
def test_v2_trainer_trains_an_epoch_from_the_resident_set():
    be = EmuRoiPoolBackend()
    cfg = _cfg(jitter=True)
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 80 * FRAME / 2 ** 30
    tr = _synthetic(cfg, n=5, seed=1, frames_per_video=(3, 8))
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    r = t.resident
    assert isinstance(r, ResidentGestureSet) and (r.capacity, r.batch_size, r.drop_last, r.jitter, r.augment) == (
        80, 2, False, (0.5, 0.3, 0.2, 0.1), False)
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append({k: v.clone() for k, v in batch.items()}), prepare(batch))[1]
    t.train_loader = None                                                     # the loader path is not taken
    t.epoch = 2
    p0 = t.model.engine.P.data.clone()
    loss, _ = t.train_epoch()
    plan = r.plan(2)
    assert loss == loss and len(seen) == len(plan) == 3 and t.num_step == 3 and not torch.equal(p0, t.model.engine.P.data)
    roi = RoiResize(64, "cpu", be)
    for batch, (videos, indices, box, crop, jitter) in zip(seen, plan):
        assert sorted(batch) == ["clip_v2", "jitter", "label"] and crop is None
        assert batch["label"].tolist() == [tr.label(v) for v in videos] and torch.equal(batch["jitter"], jitter)
        frames = torch.stack([tr.video_item(v, indices[n].tolist())["frames_pool"] for n, v in enumerate(videos)])
        assert torch.equal(batch["clip_v2"], roi(frames, box))                # (cloned BEFORE the jitter ran in place)
    assert [len(e[0]) for e in plan] == [2, 2, 1]                             # the v2 loader keeps the last, smaller batch
    assert r.bytes_uploaded == sum(tr.vframes) * FRAME and r.resident_videos == 5
    assert len(list(r.epoch(3))) == 3 and r.bytes_uploaded == sum(tr.vframes) * FRAME      # the next epoch reads nothing
    # prepare_data: the jitter is applied to the clip in place, then the two channel slices of the permuted tensor
    mm = v2.ModelManager(cfg, "cpu", be)
    batch = {k: v.clone() for k, v in seen[0].items()}
    (xs, xf), y = mm.prepare_data(batch)
    assert tuple(xs.shape) == (2, 5, 4, 64, 64) and tuple(xf.shape) == (2, 2, 4, 64, 64) and y.tolist() == seen[0]["label"].tolist()
    assert xs.untyped_storage().data_ptr() == batch["clip_v2"].untyped_storage().data_ptr() == xf.untyped_storage().data_ptr()
    assert torch.equal(xf, seen[0]["clip_v2"].permute(0, 2, 1, 3, 4)[:, 5:]) and not torch.equal(xs[:, :3], seen[0]["clip_v2"].permute(0, 2, 1, 3, 4)[:, :3])


def test_v2_trainer_refuses_what_the_resident_set_cannot_do(monkeypatch):
    be = EmuRoiPoolBackend()
    cfg = _cfg()
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 80 * FRAME / 2 ** 30
    tr = _synthetic(cfg, n=2, seed=1)
    plain = v2.SyntheticGesture(cfg, "train", num_videos=2, seed=1, h=H, w=W, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*RoiResize"):        # a set without the contract: still refused
        v2.Trainer(cfg, train_set=plain, test_set=te, device="cpu", backend=be)
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*frame_boxes"):
        v2.Trainer(cfg, train_set=plain, test_set=te, device="cpu", backend=be)
    loader = torch.utils.data.DataLoader(tr, batch_size=2)
    test_loader = torch.utils.data.DataLoader(te, batch_size=2, collate_fn=lambda x: x)
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*train_set"):
        v2.Trainer(cfg, train_loader=loader, test_loader=test_loader, device="cpu", backend=be)
    monkeypatch.setattr(v2._train.sdist, "init_process_group_from_env", lambda backend=None: (0, 2, None))
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*WORLD_SIZE"):
        v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    monkeypatch.undo()
    off = _cfg()
    t = v2.Trainer(off, train_set=tr, test_set=te, device="cpu", backend=be)  # without the switch: the loader path
    assert not hasattr(t, "resident")
