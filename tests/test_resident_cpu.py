"""The device-resident train set on CPU (include/sfk_resident.h, FramePool(capacity=), input_pipeline.ResidentTrainSet,
MODEL.RESIDENT_TRAIN, tests/emu_resident.py): the ctypes binding of the new header and its host-side rejections, the emulated
crop gather against EmuBackend.u8_normalize_crop on the materialised clips, the fixed-capacity arena, the sampling plan
replayed against DevicePreprocess, the residency and upload accounting with ample and with half capacity, and the Trainer
switch with the combinations it refuses."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from emu_resident import EmuResidentBackend, pool_gather_crop
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import (DevicePreprocess, FramePool, PadResize, ResidentTrainSet, normalize_lut,
                                                     raw_offsets, unpool_item)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "CropLHand"                                                               # 64 x 64 crops
FRAME = 64 * 64 * 21


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the binding of include/sfk_resident.h
def test_resident_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_resident.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_RESIDENT) == ["sfk_resident_abi_version", "sfk_u8_pool_gather_crop"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG,
                  _lib.SIGNATURES_POOL, _lib.SIGNATURES_RESIZE):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_RESIDENT[n]), n
    assert lib.sfk_resident_abi_version() == _lib.RESIDENT_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_RESIDENT_ABI_VERSION\s+(\d+)", src).group(1))
    body = re.search(r"typedef struct \{(.*?)\} sfk_pool_crop_desc;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._PoolCropDesc._fields_] == fields
    # the fields of sfk_pool_desc, in their order, plus crop and pad
    assert [f for f in fields if f not in ("crop", "pad")] == [f for f, _ in _lib._PoolDesc._fields_]


def test_pool_crop_desc_size_is_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_resident.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sfk_pool_crop_desc), '
                                  'offsetof(sfk_pool_crop_desc, crop), offsetof(sfk_pool_crop_desc, pad), '
                                  'offsetof(sfk_pool_crop_desc, out)); return 0; }\n')
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    size, o_crop, o_pad, o_out = (int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split())
    D = _lib._PoolCropDesc
    assert (size, o_crop, o_pad, o_out) == (ctypes.sizeof(D), D.crop.offset, D.pad.offset, D.out.offset)
    assert size == 104 == _lib.new_pool_crop_desc().struct_size


def _good_desc(pool, index, lut, crop, out):
    from video_classification_amd import _lib
    d = _lib.new_pool_crop_desc()
    d.out_dtype, d.pool, d.index, d.lut, d.out = _lib.SFK_F32, pool.data_ptr(), index.data_ptr(), lut.data_ptr(), out.data_ptr()
    d.crop, d.pad = crop.data_ptr(), 1
    d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.fill = 3, 8, 8, 0, 5, 2, 2, 127
    d.frame_stride, d.row_stride, d.pixel_pitch = 8 * 8 * 5, 8 * 5, 5
    return d


def test_pool_crop_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test): the cases of sfk_u8_pool_gather, and pad < 0"""
    pool = torch.zeros(3 * 8 * 8 * 5, dtype=torch.uint8)
    index, lut, crop = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(256), torch.zeros(2, 2, dtype=torch.int32)
    out = torch.zeros(2 * 2 * 5 * 8 * 8 + 8)
    out = out[(-out.data_ptr() // 4) % 4:]                                    # 16-byte aligned
    assert out.data_ptr() % 16 == 0
    before = out.clone()
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 96), ("struct_size", 100), ("struct_size", 112), ("pool", None),
                         ("index", None), ("lut", None), ("out", None), ("frames", 0), ("h", 0), ("w", -1), ("c", 0), ("n", 0),
                         ("t", -2), ("frame_stride", -1), ("row_stride", -40), ("c0", -1), ("pixel_pitch", 4), ("c0", 1),
                         ("fill", -1), ("fill", 256), ("out_dtype", 2), ("out_dtype", -1), ("out", out.data_ptr() + 4),
                         ("out", out.data_ptr() + 8), ("pad", -1), ("pad", -(2 ** 31))]:
        d = _good_desc(pool, index, lut, crop, out)
        setattr(d, field, value)
        assert lib.sfk_u8_pool_gather_crop(B(d), None) == -1, (field, value)
    assert lib.sfk_u8_pool_gather_crop(None, None) == -1
    for fields in [{"n": (1 << 23) // 8 + 1, "t": 1}, {"w": 60 * 1024 // 5 + 1}, {"w": 3000, "pixel_pitch": 21, "c": 21}]:
        for no_crop in (False, True):                                         # a NULL crop passes the argument checks: the
            d = _good_desc(pool, index, lut, crop, out)                       # same descriptors still fail on their SIZE (-2)
            for k, v in fields.items():
                setattr(d, k, v)
            if no_crop:
                d.crop = None
            assert lib.sfk_u8_pool_gather_crop(B(d), None) == -2, (fields, no_crop)
    assert torch.equal(out, before)


# ------------------------------------------------------------------ the emulated kernel against the materialised clips
def _video(f, s=8, p=21, seed=0):
    return torch.randint(0, 256, (f, s, s, p), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _materialise(pool, idx, fill=127):
    ext = torch.cat([pool, torch.full_like(pool[:1], fill)])
    i = idx.long()
    return ext[torch.where((i < 0) | (i >= pool.shape[0]), torch.tensor(pool.shape[0]), i)]


@pytest.mark.parametrize("s,pad", [(13, 1), (20, 2), (13, 5)])
def test_emulated_crop_gather_equals_normalize_crop_of_the_materialised_clips(s, pad):
    be = EmuResidentBackend()
    pool, lut = _video(7, s=s, seed=s), normalize_lut()
    idx = torch.tensor([[0, 1, 2], [6, -1, 3], [7, 5, 5], [2, 2, 0]], dtype=torch.int32)      # -1 and F: missing frames
    clips = _materialise(pool, idx)
    for crop in ([[0, 0]] * 4, [[pad, pad]] * 4, [[2 * pad, 2 * pad]] * 4, [[0, 2 * pad], [2 * pad, 0], [pad, 0], [1, 2 * pad - 1]]):
        crop = torch.tensor(crop, dtype=torch.int32)
        want, got = torch.empty(4, 3, 21, s, s), torch.full((4, 3, 21, s, s), -7.0)
        be.u8_normalize_crop(clips, lut, crop, pad, want)(0)
        be.u8_pool_gather_crop(pool, idx, lut, 127, crop, pad, got)(0)
        assert torch.equal(got, want), crop.tolist()
        assert torch.equal(FramePoolOf(pool, be).gather(torch.where(idx < 7, idx, -1), crop=crop, padding=pad), want)   # (F is not a slot)
    assert float(got[1, 1, 0, s - 1, s - 1]) == 0.0 and float(got[1, 1, 0, 0, s - 1]) == float(lut[127])     # padded AFTER the fill
    want, got = torch.empty(4, 3, 21, s, s), torch.full((4, 3, 21, s, s), -7.0)
    be.u8_pool_gather(pool, idx, lut, 127, want)(0)
    be.u8_pool_gather_crop(pool, idx, lut, 127, None, pad, got)(0)
    assert torch.equal(got, want)
    # a channel range, and crops far outside [0, 2*pad]: everything outside the frame is 0
    got = pool_gather_crop(pool, idx, lut, 127, torch.tensor([[-50, 3], [1, 10 ** 6], [-(2 ** 31), 2 ** 31 - 1], [pad + 2, pad - 2]]),
                           pad, 5, 15)
    assert not got[:3].any() and tuple(got.shape) == (4, 3, 15, s, s)
    assert torch.equal(got[3, 0, :, :s - 2, 2:], lut[pool[2][2:, :s - 2, 5:20].long()].permute(2, 0, 1))


def FramePoolOf(frames, be):
    pool = FramePool("cpu", be)
    pool.add(frames)
    return pool


# ------------------------------------------------------------------ FramePool(capacity=)
def test_frame_pool_with_a_capacity_never_reallocates_and_says_when_it_is_full():
    be = EmuResidentBackend()
    pool = FramePool("cpu", be, capacity=10)
    assert pool.arena is None and pool.fits(10) and not pool.fits(11)
    a = pool.add(_video(4, seed=1))
    ptr = pool.arena.data_ptr()
    assert tuple(pool.arena.shape) == (10, 8, 8, 21) and a == 0
    b = pool.add(_video(5, seed=2))
    assert b == 4 and pool.fits(1) and not pool.fits(2)
    with pytest.raises(RuntimeError, match="no room"):
        pool.add(_video(2, seed=3))
    assert pool.live == {0: 4, 4: 5} and pool.bytes_uploaded == 9 * 8 * 8 * 21      # the refused video uploaded nothing
    pool.release(a)
    assert pool.fits(4) and not pool.fits(5)                                  # first fit: the gap of 4, or the 1 at the end
    c = pool.add(_video(3, seed=4))
    assert c == 0 and pool.arena.data_ptr() == ptr and tuple(pool.arena.shape) == (10, 8, 8, 21)
    got = pool.gather(torch.tensor([[4, 8, 0, 2]], dtype=torch.int32))
    want = normalize_lut()[torch.stack([_video(5, seed=2)[0], _video(5, seed=2)[4], _video(3, seed=4)[0],
                                        _video(3, seed=4)[2]])[None].long()].permute(0, 1, 4, 2, 3)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        pool.add(_video(1, s=9))                                              # another frame shape: the arena does not move
    with pytest.raises(RuntimeError, match="no room"):
        FramePool("cpu", be, capacity=3).add(_video(4))
    with pytest.raises(ValueError):
        FramePool("cpu", be, capacity=0)
    # without a capacity: the pool doubles and carries live videos over, as before
    grow = FramePool("cpu", be)
    assert grow.fits(10 ** 9)
    assert (grow.add(_video(4, seed=1)), grow.add(_video(6, seed=2))) == (0, 4) and grow.arena.shape[0] == 10
    assert torch.equal(grow.arena[:4], _video(4, seed=1))


# ------------------------------------------------------------------ ResidentTrainSet
def _cfg(bs=2, root="/nonexistent", jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "slowfast-LHand"
    cfg.MODEL.R3D_INPUT = KEY
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


class Counting:
    """a train set seen through the three methods only, counting the calls (and hiding some frames: missing files)"""

    def __init__(self, ds, missing=()):
        self.ds, self.missing, self.calls = ds, set(missing), []

    def __len__(self):
        return len(self.ds)

    def seq_len(self, i):
        self.calls.append(("seq_len", i))
        return self.ds.seq_len(i)

    def label(self, i):
        self.calls.append(("label", i))
        return self.ds.label(i)

    def video_item(self, i, indices=None):
        self.calls.append(("video_item", i, None if indices is None else tuple(indices)))
        from video_classification_amd.input_pipeline import make_pooled_item, make_raw_pooled_item
        idx = list(range(self.ds.seq_len(i))) if indices is None else list(indices)
        make = make_raw_pooled_item if self.ds.raw else make_pooled_item
        return make(self.ds.key, [idx], self.ds.label(i), lambda k: None if (i, k) in self.missing else self.ds._video_frame(i, k))


def _frames_of_item(item, be):
    """(T, S, S, 21) uint8 frames of a video_item over a clip's indices, a missing frame as bytes of 127"""
    if KEY + "_rawpool" in item:
        hw = item["raw_hw"]
        frames = PadResize(64, "cpu", be)(item[KEY + "_rawpool"], raw_offsets(hw, 21), hw)
        item = {KEY + "_pool": frames, "windows": item["windows"], "label": item["label"]}
    return unpool_item(item)[0][KEY + "_u8"]


def _replay(r, ds, be, epochs, on_batch=None):
    """every clip epoch(e) yields is DevicePreprocess of video_item's frames at plan(e)'s indices with plan(e)'s crop"""
    pre = DevicePreprocess("cpu", be)
    for e in epochs:
        plan = r.plan(e)
        got = list(_each(r.epoch(e), on_batch))
        assert len(got) == len(plan)
        for batch, (videos, indices, crop, jitter) in zip(got, plan):
            assert sorted(batch) == sorted([KEY, "label"] + (["jitter"] if jitter is not None else []))
            assert batch["label"].tolist() == [ds.label(v) for v in videos]
            if jitter is not None:
                assert torch.equal(batch["jitter"], jitter) and tuple(jitter.shape) == (len(videos), 8)
            frames = torch.stack([_frames_of_item(ds.video_item(v, indices[n].tolist()), be) for n, v in enumerate(videos)])
            assert batch[KEY].dtype == torch.float32 and torch.equal(batch[KEY], pre(frames, crop))


def _each(it, fn):
    for b in it:
        if fn is not None:
            fn()
        yield b


@pytest.mark.parametrize("kind", ["as_uint8", "raw"])
def test_resident_train_set_replays_its_plan_and_uploads_every_frame_once(kind):
    be = EmuResidentBackend()
    cfg = _cfg(jitter=True)
    ds = v1.SyntheticChalearn(cfg, "train", num_videos=6, seed=3, frames_per_video=(2, 9), raw_side=(20, 40), **{kind: True})
    assert min(ds.vframes) < 4 < max(ds.vframes)                              # a short video wraps
    seen = Counting(ds, missing={(0, 1), (3, 0)})
    r = ResidentTrainSet(seen, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=200,
                         jitter=v1.jitter_ranges(cfg))
    other = ResidentTrainSet(ds, cfg, "cpu", be, batch_size=2, drop_last=True, seed=5, capacity_frames=9,
                             jitter=v1.jitter_ranges(cfg))
    for e in range(3):                                                        # the plan: (seed, epoch) only
        a, b = r.plan(e), other.plan(e)
        assert len(a) == len(b) == 3 and sorted(v for vs, _, _, _ in a for v in vs) == list(range(6))
        for (va, ia, ca, ja), (vb, ib, cb, jb) in zip(a, b):
            assert va == vb and torch.equal(ia, ib) and torch.equal(ca, cb) and torch.equal(ja, jb)
            assert ia.dtype == torch.int32 and tuple(ia.shape) == (2, 4) and ca.dtype == torch.int32 and tuple(ca.shape) == (2, 2)
            assert int(ca.min()) >= 0 and int(ca.max()) <= 12
            for v, row in zip(va, ia.tolist()):
                n = ds.seq_len(v)
                assert 0 <= row[0] <= max(0, n - 4) and row == [(row[0] + k) % n for k in range(4)]
    assert [v for v, _, _, _ in r.plan(0)] != [v for v, _, _, _ in r.plan(1)] or not torch.equal(r.plan(0)[0][1], r.plan(1)[0][1])
    assert ResidentTrainSet(ds, cfg, "cpu", be, batch_size=4, drop_last=False, capacity_frames=99).plan(0)[-1][0].__len__() == 2
    assert len(ResidentTrainSet(ds, cfg, "cpu", be, batch_size=4, drop_last=True, capacity_frames=99).plan(0)) == 1
    whole = sum(seen.video_item(v)[k].numel() for v in range(6) for k in (KEY + "_pool", KEY + "_rawpool") if k in seen.video_item(v))
    if kind == "as_uint8":
        assert whole == (sum(ds.vframes) - 2) * FRAME                         # the two missing frames are not uploaded
    ptr = []
    _replay(r, seen, be, [0], on_batch=lambda: ptr.append(r.pool.arena.data_ptr()))
    assert r.bytes_uploaded == whole and r.resident_videos == 6 and r.resident_frames == sum(ds.vframes) - 2
    assert r.spilled_clips == 0 and r.spill_peak == 0
    del seen.calls[:]
    for e in (1, 2):
        got = list(r.epoch(e))                                                # nothing to read: label is the only method called
        assert len(got) == 3 and {c[0] for c in seen.calls} == {"label"}
    assert r.bytes_uploaded == whole
    _replay(r, seen, be, [1, 2], on_batch=lambda: ptr.append(r.pool.arena.data_ptr()))
    assert r.bytes_uploaded == whole and len(set(ptr)) == 1
    assert not any(c[0] == "video_item" and c[2] is None for c in seen.calls)  # (the replay itself asks for the clips' frames)


@pytest.mark.parametrize("kind", ["as_uint8", "raw"])
def test_resident_train_set_with_half_the_capacity_spills_the_rest(kind):
    be = EmuResidentBackend()
    cfg = _cfg()
    ds = v1.SyntheticChalearn(cfg, "train", num_videos=8, seed=4, frames_per_video=(2, 12), raw_side=(20, 40), **{kind: True})
    assert min(ds.vframes) < 4
    cap = sum(ds.vframes) // 2 + 2 * 4                                        # about half the frames, plus the spill region

    def run():
        seen = Counting(ds)
        r = ResidentTrainSet(seen, cfg, "cpu", be, batch_size=2, drop_last=False, seed=1, capacity_frames=cap)
        assert (r.resident_slots, r.spill_slots) == (cap - 8, 8)
        log = []
        for e in range(3):
            before, ptr = r.bytes_uploaded, None
            del seen.calls[:]
            def check():
                assert sum(r.pool.live.values()) <= cap and r.spill_peak <= 8
            _replay(r, seen, be, [e], on_batch=check)
            resident = sorted(v for v, ok in r._resident.items() if ok)
            log.append((resident, r.bytes_uploaded - before, r.spilled_clips, dict(r.pool.live)))
            assert sorted(r.pool.live.values()) == sorted(r._rows[v].ge(0).sum().item() for v in resident)    # spills released
        return r, log

    (r, log), (_, again) = run(), run()
    assert log == again                                                       # the same videos resident, the same uploads
    resident = log[0][0]
    assert 0 < len(resident) < 8 and log[1][0] == log[2][0] == resident and r.resident_videos == len(resident)
    assert sum(ds.vframes[v] for v in resident) == r.resident_used <= r.resident_slots == r.resident_frames + (
        r.resident_slots - r.resident_used)
    # the rule, replayed: first come, first resident, in plan order
    used, want = 0, []
    for videos, _, _, _ in r.plan(0):
        for v in videos:
            if used + ds.vframes[v] <= cap - 8:
                used += ds.vframes[v]
                want.append(v)
    assert sorted(want) == resident
    frame_bytes = lambda v, ks: sum(ds.video_item(v, ks)[k].numel() for k in (KEY + "_pool", KEY + "_rawpool") if k in ds.video_item(v, ks))
    for e in (1, 2):                                                          # exactly the distinct frames of the spilled clips
        spilled = [(v, sorted(set(row.tolist()))) for vs, idx, _, _ in r.plan(e) for v, row in zip(vs, idx) if v not in resident]
        assert log[e][1] == sum(frame_bytes(v, ks) for v, ks in spilled) > 0 and log[e][2] == len(spilled) == 8 - len(resident)
    assert 0 < r.spill_peak <= 8
    with pytest.raises(ValueError, match="no resident slot"):
        ResidentTrainSet(ds, cfg, "cpu", be, batch_size=2, capacity_frames=8)
    with pytest.raises(ValueError, match="seq_len"):
        ResidentTrainSet(torch.utils.data.TensorDataset(torch.zeros(3)), cfg, "cpu", be, batch_size=2, capacity_frames=99)
    cfg.MODEL.RESIDENT_GB = 20 * FRAME / 2 ** 30                              # the default capacity: floor(GB * 2^30 / (S*S*21))
    assert ResidentTrainSet(ds, cfg, "cpu", be, batch_size=2).capacity == 20


def test_chalearn_video_frames_u8_offers_the_three_methods(tmp_path):
    import numpy as np
    cfg = _cfg(root=tmp_path)
    labels = []
    for i, f in enumerate((6, 3)):
        rel = f"train/001/M_{i:05d}"
        (tmp_path / "2_Images" / rel).mkdir(parents=True)
        (tmp_path / KEY / rel).mkdir(parents=True)
        for k in range(f):
            (tmp_path / "2_Images" / rel / f"{k * 5:05d}.jpg").write_bytes(b"")
            if (i, k) != (0, 2):
                (tmp_path / KEY / rel / f"{k * 5:05d}.jpg").write_bytes(b"")
        labels.append((rel + ".avi", rel + ".avi", i + 4))
    calls = []

    def read_frame(path, size=None):
        calls.append(str(path))
        if not os.path.exists(path):
            return None
        k = int(os.path.basename(path)[:5]) // 5
        return np.full((size or 30, size or 20 + k, 21), k, dtype=np.uint8)
    ds = v1.ChalearnVideoFramesU8(cfg, "train", labels, read_frame)
    assert (ds.seq_len(0), ds.seq_len(1), ds.label(0), ds.label(1)) == (6, 3, 3, 4) and not calls
    it = ds.video_item(0)
    assert sorted(it) == [KEY + "_pool", "label", "windows"] and it["label"] == 3 and len(calls) == 6
    assert it["windows"].tolist() == [[0, 1, -1, 2, 3, 4]] and it[KEY + "_pool"][:, 0, 0, 0].tolist() == [0, 1, 3, 4, 5]
    del calls[:]
    it = ds.video_item(1, [2, 0, 1, 2])
    assert it["windows"].tolist() == [[2, 0, 1, 2]] and len(calls) == 3 and it[KEY + "_pool"][:, 0, 0, 0].tolist() == [0, 1, 2]
    raw = v1.ChalearnVideoFramesU8(cfg, "train", labels, read_frame, resize="device").video_item(0, [1, 2, 3])
    assert sorted(raw) == [KEY + "_rawpool", "label", "raw_hw", "windows"] and raw["windows"].tolist() == [[0, -1, 1]]
    assert raw["raw_hw"].tolist() == [[30, 21], [30, 23]]
    r = ResidentTrainSet(ds, cfg, "cpu", EmuResidentBackend(), batch_size=2, capacity_frames=40)
    (batch,) = list(r.epoch(0))
    assert tuple(batch[KEY].shape) == (2, 4, 21, 64, 64) and sorted(batch["label"].tolist()) == [3, 4]
    assert r.bytes_uploaded == (5 + 3) * FRAME and r.resident_frames == 8


# ------------------------------------------------------------------ the Trainer switch
def test_config_defaults():
    from video_classification_amd.config import get_cfg
    assert get_cfg().MODEL.RESIDENT_TRAIN is False and get_cfg().MODEL.RESIDENT_GB == 32.0


def _sets(cfg, n=4):
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=n, seed=1, as_uint8=True, frames_per_video=(3, 8))
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2, pooled=True, frames_per_video=(3, 6))
    return tr, te


def test_trainer_trains_an_epoch_from_the_resident_set():
    cfg = _cfg(jitter=True)
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 60 * FRAME / 2 ** 30
    tr, te = _sets(cfg)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuResidentBackend())
    r = t.resident
    assert isinstance(r, ResidentTrainSet) and (r.capacity, r.batch_size, r.drop_last, r.jitter) == (60, 2, True, (0.5, 0.3, 0.2, 0.1))
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append(batch), prepare(batch))[1]
    t.train_loader = None                                                     # the loader path is not taken
    t.epoch = 2
    loss, _ = t.train_epoch()
    plan = r.plan(2)
    assert loss == loss and len(seen) == len(plan) == 2 and t.num_step == 2
    for batch, (videos, _, _, jitter) in zip(seen, plan):
        assert sorted(batch) == [KEY, "jitter", "label"] and tuple(batch[KEY].shape) == (2, 4, 21, 64, 64)
        assert batch["label"].tolist() == [tr.label(v) for v in videos] and torch.equal(batch["jitter"], jitter)
    assert r.bytes_uploaded == sum(tr.vframes) * FRAME and r.resident_videos == 4
    assert len(list(r.epoch(3))) == 2 and r.bytes_uploaded == sum(tr.vframes) * FRAME      # the next epoch reads nothing


def test_trainer_without_the_switch_takes_the_loader_path():
    cfg = _cfg()
    tr, te = _sets(cfg, n=2)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuResidentBackend())
    assert not hasattr(t, "resident")
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append(sorted(batch)), prepare(batch))[1]
    t.train_epoch()
    assert seen == [[KEY + "_u8", "crop", "label"]]


def test_trainer_refuses_what_the_resident_set_cannot_do(monkeypatch):
    from video_classification_amd import gesture_v2 as v2
    be = EmuResidentBackend()
    cfg = _cfg()
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 60 * FRAME / 2 ** 30
    tr, te = _sets(cfg, n=2)
    loader = torch.utils.data.DataLoader(tr, batch_size=2)
    test_loader = torch.utils.data.DataLoader(te, batch_size=2, collate_fn=lambda x: x)
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*train_set"):
        v1.Trainer(cfg, train_loader=loader, test_loader=test_loader, device="cpu", backend=be)

    class Plain(torch.utils.data.Dataset):
        def __len__(self):
            return len(tr)

        def __getitem__(self, i):
            return tr[i]
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*seq_len"):
        v1.Trainer(cfg, train_set=Plain(), test_set=te, device="cpu", backend=be)
    with pytest.raises(ValueError, match="as_uint8"):                         # a float32 set has no frames to keep
        v1.SyntheticChalearn(cfg, "train", num_videos=2).video_item(0)
    monkeypatch.setattr(v1.sdist, "init_process_group_from_env", lambda backend=None: (0, 2, None))
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*WORLD_SIZE"):
        v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    monkeypatch.undo()
    res2d = _cfg()
    res2d.MODEL.RESIDENT_TRAIN = True
    res2d.MODEL.NAME = "res2d"
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*res2d"):
        v1.Trainer(res2d, train_set=tr, test_set=te, device="cpu", backend=be)
    g = _cfg()
    g.MODEL.RESIDENT_TRAIN = True
    g.MODEL.NAME = "gesture-v2"
    g.MODEL.INPUT_SIZE = 64
    gtr = v2.SyntheticGesture(g, "train", num_videos=2, seed=1, h=48, w=64, min_box=8)
    gte = v2.SyntheticGesture(g, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    with pytest.raises(ValueError, match="RESIDENT_TRAIN.*RoiResize"):
        v2.Trainer(g, train_set=gtr, test_set=gte, device="cpu", backend=be)
