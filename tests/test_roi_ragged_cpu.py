"""The box-cropped resident v2 train set on CPU (include/sfk_roi_ragged.h, input_pipeline.BoxArena, ResidentGestureSet(store='box'),
MODEL.RESIDENT_STORE on gesture_v2.Trainer, tests/emu_roi_ragged.py): the ctypes binding of the new header and its host-side
rejections, the byte arena's placement and its two host checks, the 'box' store against the 'frame' store batch for batch, and
the upload accounting against a sum made on the host from the plan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from emu_roi_ragged import EmuRoiRaggedBackend, materialise_ragged
from emu_v2 import roi_resize_ref
from video_classification_amd import gesture_v2 as v2
from video_classification_amd.input_pipeline import NO_BOX, BoxArena, FramePool, ResidentGestureSet, RoiResize, byte_lut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
FRAME = H * W * 7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the binding of include/sfk_roi_ragged.h
def test_roi_ragged_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_roi_ragged.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_ROI_RAGGED) == ["sfk_roi_ragged_abi_version", "sfk_roi_resize_ragged"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG,
                  _lib.SIGNATURES_POOL, _lib.SIGNATURES_RESIZE, _lib.SIGNATURES_RESIDENT, _lib.SIGNATURES_ROI_POOL):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_ROI_RAGGED[n]), n
    assert lib.sfk_roi_ragged_abi_version() == _lib.ROI_RAGGED_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_ROI_RAGGED_ABI_VERSION\s+(\d+)", src).group(1))
    body = re.search(r"typedef struct \{(.*?)\} sfk_roi_ragged_desc;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._RoiRaggedDesc._fields_] == fields
    # sfk_roi_desc with its source addressing (src, the five strides, h and w) replaced by the arena's
    roi = [f for f, _ in _lib._RoiDesc._fields_ if f not in ("src", "sn", "st", "sh", "sw", "sc", "h", "w", "reserved0")]
    arena = ("arena", "arena_bytes", "pixel_pitch", "c0", "max_h", "max_w", "offset", "hw", "fill")
    assert sorted(f for f in fields if f not in arena) == sorted(roi)


def test_roi_ragged_desc_size_is_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    names = ("arena", "arena_bytes", "max_w", "offset", "hw", "crop", "fill", "dst", "dh", "c_off")
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_roi_ragged.h"\n'
                                  'int main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(sfk_roi_ragged_desc), '
                                  + ", ".join(f"offsetof(sfk_roi_ragged_desc, {n})" for n in names) + "); return 0; }\n")
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib._RoiRaggedDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in names]
    assert got[0] == 168 == _lib.new_roi_ragged_desc().struct_size


def _good_desc(arena, offset, hw, lut, box, crop, out):
    from video_classification_amd import _lib
    d = _lib.new_roi_ragged_desc()
    d.antialias, d.arena, d.arena_bytes, d.offset, d.hw = 1, arena.data_ptr(), arena.numel(), offset.data_ptr(), hw.data_ptr()
    d.lut, d.box, d.crop = lut.data_ptr(), box.data_ptr(), crop.data_ptr()
    d.pixel_pitch, d.c0, d.c, d.n, d.t, d.max_h, d.max_w, d.pad, d.fill = 7, 0, 7, 1, 2, 240, 320, 19, 127
    d.out_h, d.out_w, d.dst_dtype, d.dst, d.c_off = 192, 192, _lib.SFK_F32, out.data_ptr(), 0
    d.dn, d.dt, d.dc, d.dh = 2 * 7 * 192 * 192, 7 * 192 * 192, 192 * 192, 192
    return d


def test_roi_ragged_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test): what sfk_roi_resize_pool rejects, with its codes,
    made on (max_h, max_w), and what the header adds for the arena"""
    arena = torch.zeros(64, dtype=torch.uint8)
    assert arena.data_ptr() % 4 == 0
    offset, hw = torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    lut, box = torch.zeros(256), torch.zeros(4, dtype=torch.int32)
    crop, out = torch.zeros(2, dtype=torch.int32), torch.full((8,), 3.0)
    B = ctypes.byref
    assert _good_desc(arena, offset, hw, lut, box, crop, out).struct_size == 168
    for field, value in [("struct_size", 8), ("struct_size", 164), ("struct_size", 176), ("arena", None), ("offset", None),
                         ("hw", None), ("lut", None), ("box", None), ("dst", None), ("arena_bytes", 0), ("arena_bytes", -4),
                         ("arena_bytes", 62), ("arena", arena.data_ptr() + 1), ("arena", arena.data_ptr() + 2), ("n", 0),
                         ("t", -1), ("max_h", 0), ("max_w", -3), ("c", 0), ("out_h", 0), ("out_w", -1), ("c0", -1), ("c0", 1),
                         ("pixel_pitch", 6), ("fill", -1), ("fill", 256), ("dn", -1), ("dh", -1), ("antialias", 2), ("pad", -1),
                         ("c_off", -1), ("dst_dtype", 7)]:
        d = _good_desc(arena, offset, hw, lut, box, crop, out)
        setattr(d, field, value)
        assert lib.sfk_roi_resize_ragged(B(d), None) == -1, (field, value)
    assert lib.sfk_roi_resize_ragged(None, None) == -1
    # SFK_ERR_UNSUPPORTED, as sfk_roi_resize_pool, on (max_h, max_w): 240/29 and 320/39 > SFK_ROI_MAX_RATIO
    for fields in [{"c": 17, "pixel_pitch": 17}, {"out_h": 29}, {"out_w": 39}, {"pixel_pitch": 4097}, {"out_h": 29, "crop": None},
                   {"max_h": 192 * 8 + 1}, {"max_w": 192 * 8 + 1}]:
        d = _good_desc(arena, offset, hw, lut, box, crop, out)
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.sfk_roi_resize_ragged(B(d), None) == -2, fields
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------ BoxArena on the emulated backend
def test_box_arena_places_first_fit_at_aligned_offsets_and_never_moves():
    be = EmuRoiRaggedBackend()
    g = torch.Generator().manual_seed(7)
    a, b, c = (torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((3, 5, 9, 7), (2, 11, 3, 7), (1, 4, 4, 7)))
    arena = BoxArena(3000 + 13, "cpu", be)
    assert arena.capacity == 3008 and arena.arena is None and arena.fits(3008) and not arena.fits(3009) and not arena.fits(0)
    base_a = arena.add(a)                                                     # 945 bytes -> [0, 960)
    ptr = arena.arena.data_ptr()
    base_b, base_c = arena.add(b), arena.add(c)                               # 462 -> [960, 1424); 112 -> [1424, 1536)
    assert (base_a, base_b, base_c) == (0, 960, 1424) and arena.arena.numel() == 3008
    assert arena.live == {0: (3, 5, 9, 7), 960: (2, 11, 3, 7), 1424: (1, 4, 4, 7)}
    assert arena.bytes_uploaded == 945 + 462 + 112
    assert torch.equal(arena.arena[960:960 + 462].view(2, 11, 3, 7), b) and torch.equal(arena.arena[:945].view(3, 5, 9, 7), a)
    assert arena.fits(3008 - 1536) and not arena.fits(3008 - 1536 + 1)
    arena.release(base_b)
    assert arena.fits(464) and arena.fits(3008 - 1536)
    d = torch.randint(0, 256, (4, 4, 4, 7), generator=g, dtype=torch.uint8)   # 448 bytes: first fit is b's hole
    e = torch.randint(0, 256, (1, 5, 14, 7), generator=g, dtype=torch.uint8)  # 490 bytes: not the 16 left of it, the tail
    assert arena.add(d) == 960 and arena.add(e) == 1536 and arena.arena.data_ptr() == ptr
    with pytest.raises(RuntimeError, match="BoxArena: no room"):
        arena.add(torch.zeros(1, 10, 21, 7, dtype=torch.uint8))               # 1470 > 3008 - 2032
    assert arena.bytes_uploaded == 945 + 462 + 112 + 448 + 490 and sorted(arena.live) == [0, 960, 1424, 1536]
    off = arena.offsets(960, torch.tensor([[0, 3, -1], [2, 2, 1]]))
    assert off.dtype == torch.int64 and off.tolist() == [[960, 960 + 3 * 112, -1], [960 + 224, 960 + 224, 960 + 112]]
    with pytest.raises(ValueError, match="window index"):
        arena.offsets(960, torch.tensor([[4]]))
    with pytest.raises(ValueError, match="capacity"):
        BoxArena(15, "cpu", be)


def test_box_arena_roi_gather_is_roi_resize_of_each_clips_frames_and_checks_its_tables():
    be = EmuRoiRaggedBackend()
    g = torch.Generator().manual_seed(3)
    whole = torch.randint(0, 256, (4, H, W, 7), generator=g, dtype=torch.uint8)
    rect = (5, 3, 44, 32)                                                     # x1, y1, x2, y2
    part = whole[:, 3:32, 5:44].contiguous()
    other = torch.randint(0, 256, (3, 17, 23, 7), generator=g, dtype=torch.uint8)
    arena = BoxArena(1 << 20, "cpu", be)
    pool = FramePool("cpu", be)
    pool.add(whole)
    base_w, base_p, base_o = arena.add(whole), arena.add(part), arena.add(other)
    off = torch.stack([arena.offsets(base_w, torch.tensor([[0, 1, -1, 3]]))[0], arena.offsets(base_p, torch.tensor([[0, 1, -1, 3]]))[0],
                       arena.offsets(base_o, torch.tensor([[2, 2, 0, 1]]))[0]])
    hw = torch.tensor([[H, W], [29, 39], [17, 23]], dtype=torch.int32)
    full = torch.tensor([9, 4, 40, 30], dtype=torch.int32)                    # the same box, in the frame and in the rectangle
    box = torch.stack([full, full - torch.tensor([5, 3, 5, 3], dtype=torch.int32), torch.tensor([0, 0, 23, 17], dtype=torch.int32)])
    crop = torch.tensor([[0, 6], [0, 6], [6, 0]], dtype=torch.int32)
    for aa in (True, False):
        for cr in (None, crop):
            got = arena.roi_gather(off, hw, box, 32, torch.float32, aa, crop=cr)
            assert torch.equal(got[0], got[1])                                # the claim: a containing rectangle changes nothing
            want = pool.roi_gather(torch.tensor([[0, 1, -1, 3]], dtype=torch.int32), full[None], 32, torch.float32, aa,
                                   crop=None if cr is None else cr[:1])
            assert torch.equal(got[:1], want)
            clip = materialise_ragged(arena.arena, off[2], hw[2], 127, (H, W))
            assert torch.equal(clip[0, 0], other[2]) and torch.equal(clip[0, 3], other[1])
            assert torch.equal(got[2:], RoiResize(32, "cpu", be, antialias=aa)(clip, box[2:], None if cr is None else cr[2:]))
            assert torch.equal(got[2:], roi_resize_ref(clip, byte_lut(), box[2:], 32, 32, aa, None if cr is None else cr[2:], 3))
    out = torch.full((3, 4, 7, 32, 32), -7.0)
    assert arena.roi_gather(off, hw, box, 32, crop=crop, padding=3, out=out) is out
    assert torch.equal(out, arena.roi_gather(off, hw, box, 32, crop=crop))
    assert arena.roi_gather(off, hw, box, 32, torch.bfloat16).dtype == torch.bfloat16
    # an offset that is not the start of a live frame of the clip's shape
    for bad in (off[0, 0] + 1, off[1, 1] + 7, base_o + 3 * 17 * 23 * 7, -2, arena.capacity):
        o = off.clone()
        o[0, 0] = bad
        with pytest.raises(ValueError, match="roi_gather: offset"):
            arena.roi_gather(o, hw, box, 32)
    with pytest.raises(ValueError, match="roi_gather: offset"):               # a live frame, but of another rectangle
        arena.roi_gather(off[[1, 0, 2]], hw, box, 32)
    # a box outside its rectangle
    for n, bad in ((1, (0, 0, 40, 29)), (1, (0, 0, 39, 30)), (0, (-1, 0, 5, 5)), (2, (4, 4, 4, 9)), (2, (0, 9, 5, 9)), (0, (0, -2, 5, 5))):
        b = box.clone()
        b[n] = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(ValueError, match="roi_gather: box"):
            arena.roi_gather(off, hw, b, 32)
    arena.release(base_p)
    with pytest.raises(ValueError, match="roi_gather: offset"):               # no longer live
        arena.roi_gather(off, hw, box, 32)
    assert tuple(arena.roi_gather(off[2:], hw[2:], box[2:], 16).shape) == (1, 4, 7, 16, 16)


# ------------------------------------------------------------------ ResidentGestureSet(store='box') against store='frame'
def _cfg(bs=2, jitter=False, t=4):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
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


def _rect(ds, v):
    """R_v on the host: the union of the video's frame boxes (NO_BOX rows drop out of min / max), clamped to the frame"""
    b = ds.frame_boxes(v)
    return max(0, int(b[:, 0].min())), max(0, int(b[:, 1].min())), min(W, int(b[:, 2].max())), min(H, int(b[:, 3].max()))


def _ceil16(v):
    return (v + 15) // 16 * 16


def _spill_region(bs, t=4):
    return bs * (t * FRAME + 16)


def _assert_same_plan(pa, pb):
    assert len(pa) == len(pb)
    for ea, eb in zip(pa, pb):
        assert ea[0] == eb[0] and len(ea) == len(eb) == 5
        for x, y in zip(ea[1:], eb[1:]):
            assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("augment,jitter", [(False, False), (True, True)])
@pytest.mark.parametrize("room", ["ample", "half", "none"])
def test_box_store_yields_the_frame_stores_batches_bit_for_bit(augment, jitter, room):
    be = EmuRoiRaggedBackend()
    cfg = _cfg(jitter=jitter)
    cfg.MODEL.RESIZE_ANTIALIAS = not augment
    ds = _synthetic(cfg, n=7, seed=4, frames_per_video=(2, 11))
    jit = (0.5, 0.3, 0.2, 0.1) if jitter else None
    costs = [_ceil16(ds.seq_len(v) * (r[3] - r[1]) * (r[2] - r[0]) * 7) for v in range(7) for r in [_rect(ds, v)]]
    nbytes = _spill_region(2) + {"ample": sum(costs), "half": sum(costs) // 2, "none": 16}[room]
    kw = dict(batch_size=2, drop_last=False, seed=9, jitter=jit, augment=augment)
    fr = ResidentGestureSet(ds, cfg, "cpu", be, capacity_frames=200, **kw)
    bx = ResidentGestureSet(ds, cfg, "cpu", be, store="box", capacity_bytes=nbytes, **kw)
    assert (fr.store, bx.store) == ("frame", "box") and isinstance(bx.pool, BoxArena) and isinstance(fr.pool, FramePool)
    assert (bx.capacity, bx.spill_slots, bx.resident_slots) == (nbytes, _spill_region(2), nbytes - _spill_region(2))
    for e in range(3):
        _assert_same_plan(fr.plan(e), bx.plan(e))
        a, b = list(fr.epoch(e)), list(bx.epoch(e))
        assert len(a) == len(b) == 4
        for x, y in zip(a, b):
            assert sorted(x) == sorted(y) == sorted(["clip_v2", "label"] + (["jitter"] if jitter else []))
            for k in x:
                assert torch.equal(x[k], y[k]), (e, k)
            assert tuple(y["clip_v2"].shape[1:]) == (4, 7, 64, 64)
    resident = sorted(v for v, ok in bx._resident.items() if ok)
    assert {"ample": len(resident) == 7, "half": 0 < len(resident) < 7, "none": resident == []}[room]
    assert bx.resident_videos == len(resident) and bx.resident_used == sum(costs[v] for v in resident) <= bx.resident_slots
    assert bx.resident_bytes_used == sum(ds.seq_len(v) * (r[3] - r[1]) * (r[2] - r[0]) * 7 for v in resident for r in [_rect(ds, v)])
    assert fr.resident_bytes_used == sum(ds.vframes) * FRAME and bx.resident_frames == sum(ds.seq_len(v) for v in resident)
    assert sorted(bx.pool.live.values()) == sorted((ds.seq_len(v), r[3] - r[1], r[2] - r[0], 7) for v in resident for r in [_rect(ds, v)])
    assert bx.spilled_clips == 7 - len(resident) and bx.spill_peak <= 8 and (bx.spill_peak > 0) == (room != "ample")
    assert bx.bytes_uploaded < fr.bytes_uploaded or room == "none"


@pytest.mark.parametrize("room", ["ample", "half", "none"])
def test_box_store_uploads_what_the_plan_says_and_nothing_once_resident(room):
    be = EmuRoiRaggedBackend()
    cfg = _cfg()
    ds = _synthetic(cfg, n=8, seed=4, frames_per_video=(2, 12))
    rects = [_rect(ds, v) for v in range(8)]
    area = [(r[3] - r[1]) * (r[2] - r[0]) for r in rects]
    assert all(0 < a < H * W for a in area)
    costs = [_ceil16(ds.seq_len(v) * area[v] * 7) for v in range(8)]
    budget = {"ample": sum(costs), "half": sum(costs) // 2, "none": min(costs) - 16}[room]
    r = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, seed=1, store="box", capacity_bytes=_spill_region(2) + budget)
    used, resident, loaded = 0, set(), set()                                  # the rule, replayed: first come, first resident
    for entry in r.plan(0):
        for v in entry[0]:
            if used + costs[v] <= budget:
                used += costs[v]
                resident.add(v)
    assert {"ample": len(resident) == 8, "half": 0 < len(resident) < 8, "none": not resident}[room]
    ptr = set()
    for e in range(3):
        want = 0
        for videos, indices, box, crop, jitter in r.plan(e):
            for n, v in enumerate(videos):
                if v in resident:
                    want += 0 if v in loaded else ds.seq_len(v) * area[v] * 7
                    loaded.add(v)
                else:
                    x1, y1, x2, y2 = box[n].tolist()
                    want += len(set(indices[n].tolist())) * (y2 - y1) * (x2 - x1) * 7
        before = r.bytes_uploaded
        for _ in r.epoch(e):
            ptr.add(r.pool.arena.data_ptr())
            assert sum(BoxArena._span(s) for s in r.pool.live.values()) <= r.capacity
        assert r.bytes_uploaded - before == want, (e, room)
        assert (want == 0) == (room == "ample" and e > 0)
        assert sorted(v for v, ok in r._resident.items() if ok) == sorted(resident) and r.resident_used == used
        assert r.spilled_clips == 8 - len(resident)
    assert len(ptr) == 1                                                      # allocated once, never moved
    with pytest.raises(ValueError, match="no resident byte"):
        ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, store="box", capacity_bytes=_spill_region(2))
    with pytest.raises(ValueError, match="store"):
        ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, store="rows")
    with pytest.raises(ValueError, match="capacity_bytes"):
        ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, capacity_bytes=1 << 20)
    cfg.MODEL.RESIDENT_GB = (_spill_region(2) + 4096 + 5) / 2 ** 30         # the default capacity: floor(GB * 2^30) bytes
    d = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, store="box")
    assert (d.capacity, d.resident_slots) == (_spill_region(2) + 4096, 4096)
    assert ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, store="box", capacity_frames=20).capacity == 20 * FRAME


class Boxless:
    """a train set one of whose videos has no part box in any frame"""

    def __init__(self, ds, boxless):
        self.ds, self.boxless, self.reads = ds, boxless, 0

    def __len__(self):
        return len(self.ds)

    def seq_len(self, i):
        return self.ds.seq_len(i)

    def label(self, i):
        return self.ds.label(i)

    def frame_boxes(self, i):
        b = self.ds.frame_boxes(i)
        return torch.tensor([NO_BOX] * b.shape[0], dtype=torch.int32) if i == self.boxless else b

    def video_item(self, i, indices=None):
        self.reads += 1
        return self.ds.video_item(i, indices)


def test_a_video_without_any_box_is_spill_only_and_plan_raises_before_any_upload():
    be = EmuRoiRaggedBackend()
    cfg = _cfg()
    ds = Boxless(_synthetic(cfg, n=4, seed=2), 2)
    r = ResidentGestureSet(ds, cfg, "cpu", be, batch_size=2, store="box", capacity_bytes=_spill_region(2) + 50 * FRAME)
    assert ds.reads == 1                                                      # the frame shape: one frame, once
    assert r.video_rect(2) is None and r._cost(2) is None and r._decide(2) is False and r.video_rect(0) == _rect(ds.ds, 0)
    with pytest.raises(ValueError, match="video 2"):
        r.plan(0)
    with pytest.raises(ValueError, match="video 2"):
        next(iter(r.epoch(0)))
    assert r.bytes_uploaded == 0 and ds.reads == 1 and r.pool.arena is None


# ------------------------------------------------------------------ the v2 Trainer switch
def test_v2_trainer_passes_resident_store_through_and_trains_the_same():
    from video_classification_amd.config import get_cfg
    assert get_cfg().MODEL.RESIDENT_STORE == "frame"
    be = EmuRoiRaggedBackend()
    out = {}
    for store in ("frame", "box"):
        torch.manual_seed(0)
        cfg = _cfg(jitter=True)
        cfg.MODEL.RESIDENT_TRAIN = True
        cfg.MODEL.RESIDENT_STORE = store
        cfg.MODEL.RESIDENT_GB = 80 * FRAME / 2 ** 30
        tr = _synthetic(cfg, n=5, seed=1, frames_per_video=(3, 8))
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
        t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
        r = t.resident
        assert isinstance(r, ResidentGestureSet) and r.store == store and (r.batch_size, r.drop_last, r.augment) == (2, False, False)
        assert isinstance(r.pool, BoxArena if store == "box" else FramePool)
        t.train_loader = None
        t.epoch = 2
        loss, _ = t.train_epoch()
        out[store] = (loss, t.model.engine.P.data.clone(), r.bytes_uploaded, r.resident_videos)
        assert len(list(r.epoch(3))) == 3 and r.bytes_uploaded == out[store][2]                # the next epoch reads nothing
    assert out["box"][0] == out["frame"][0] and torch.equal(out["box"][1], out["frame"][1])
    assert out["box"][3] == out["frame"][3] == 5 and out["box"][2] < out["frame"][2] == sum(tr.vframes) * FRAME
    assert t.resident.capacity == 80 * FRAME // 16 * 16
