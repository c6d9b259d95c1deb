"""The pooled evaluation input on CPU (include/sfk_pool.h, input_pipeline.uniform_windows / unpool_item / FramePool,
tests/emu_pool.py): the ctypes binding of the new header and its host-side rejections, the window table against a literal
transcription of the reference's uniform_sampling, the pooled item contract, FramePool's upload-once accounting across batches,
Trainer.run_eval on pooled videos against the same videos as lists of clips, and the frames loader ChalearnVideoFramesU8."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from emu_pool import EmuPoolBackend
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import (DevicePreprocess, FramePool, make_pooled_item, normalize_lut,
                                                     uniform_windows, unpool_item)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the binding of include/sfk_pool.h
def test_pool_table_matches_its_header(lib):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_pool.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_POOL) == ["sfk_pool_abi_version", "sfk_u8_pool_gather"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_POOL[n]), n
    assert lib.sfk_pool_abi_version() == _lib.POOL_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_POOL_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.POOL_MAX_ROW_BYTES == 60 * 1024 and re.search(r"#define\s+SFK_POOL_MAX_ROW_BYTES\s+\(60 \* 1024\)", src)
    body = re.search(r"typedef struct \{(.*?)\} sfk_pool_desc;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._PoolDesc._fields_] == fields


def test_pool_desc_size_is_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_pool.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(sfk_pool_desc), offsetof(sfk_pool_desc, index), '
                                  'offsetof(sfk_pool_desc, fill), offsetof(sfk_pool_desc, out)); return 0; }\n')
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    size, o_index, o_fill, o_out = (int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split())
    D = _lib._PoolDesc
    assert (size, o_index, o_fill, o_out) == (ctypes.sizeof(D), D.index.offset, D.fill.offset, D.out.offset)
    assert size == 96 == _lib.new_pool_desc().struct_size


def _good_pool(pool, index, lut, out):
    from video_classification_amd import _lib
    d = _lib.new_pool_desc()
    d.out_dtype, d.pool, d.index, d.lut, d.out = _lib.SFK_F32, pool.data_ptr(), index.data_ptr(), lut.data_ptr(), out.data_ptr()
    d.frames, d.h, d.w, d.c0, d.c, d.n, d.t, d.fill = 3, 8, 8, 0, 5, 2, 2, 127
    d.frame_stride, d.row_stride, d.pixel_pitch = 8 * 8 * 5, 8 * 5, 5
    return d


def test_pool_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    pool = torch.zeros(3 * 8 * 8 * 5, dtype=torch.uint8)
    index, lut = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(256)
    out = torch.zeros(2 * 2 * 5 * 8 * 8 + 8)
    out = out[(-out.data_ptr() // 4) % 4:]                                    # 16-byte aligned
    assert out.data_ptr() % 16 == 0
    before = out.clone()
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 92), ("struct_size", 104), ("pool", None), ("index", None),
                         ("lut", None), ("out", None), ("frames", 0), ("h", 0), ("w", -1), ("c", 0), ("n", 0), ("t", -2),
                         ("frame_stride", -1), ("row_stride", -40), ("c0", -1), ("pixel_pitch", 4), ("c0", 1),
                         ("fill", -1), ("fill", 256), ("out_dtype", 2), ("out_dtype", -1), ("out", out.data_ptr() + 4),
                         ("out", out.data_ptr() + 8)]:
        d = _good_pool(pool, index, lut, out)
        setattr(d, field, value)
        assert lib.sfk_u8_pool_gather(B(d), None) == -1, (field, value)
    assert lib.sfk_u8_pool_gather(None, None) == -1
    for fields in [{"n": (1 << 23) // 8 + 1, "t": 1}, {"w": 60 * 1024 // 5 + 1}, {"w": 3000, "pixel_pitch": 21, "c": 21}]:
        d = _good_pool(pool, index, lut, out)                                 # 2^23 + 8 workgroups; rows of 61445 and 62 979 + 21 bytes
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.sfk_u8_pool_gather(B(d), None) == -2, fields
    assert torch.equal(out, before)


# ------------------------------------------------------------------ the windows
def uniform_sampling_transcribed(seq_len, clip_len):
    """dataset/chalearn_dataset.py:123-140 of the reference, literally, with random.randint(0, 0) written as the 0 it returns
    (uniform_sampling reaches random_sampling only with seq_len <= clip_len, where possible_start_idx is 0)"""
    def random_sampling(seq_len, clip_len):
        possible_start_idx = seq_len - clip_len
        possible_start_idx = max(0, possible_start_idx)
        assert possible_start_idx == 0
        start_idx = 0
        clip_indices = range(start_idx, start_idx + clip_len)
        clip_indices = [i % seq_len for i in clip_indices]
        return clip_indices
    clips = []
    if (seq_len <= clip_len):
        clips.append(random_sampling(seq_len, clip_len))
    else:
        t = 0
        for t in range(0, seq_len - clip_len, 4):
            clip_indices = range(t, t + clip_len)
            clips.append(clip_indices)
    return clips


def test_uniform_windows_equal_the_reference_loop():
    for clip_len in (4, 8, 20):
        for seq_len in range(1, 61):
            got = uniform_windows(seq_len, clip_len)
            want = [list(c) for c in uniform_sampling_transcribed(seq_len, clip_len)]
            assert got.dtype == torch.int32 and got.tolist() == want, (seq_len, clip_len)
    assert uniform_windows(11, 4)[:, 0].tolist() == [0, 4] and uniform_windows(11, 4).shape == (2, 4)     # frames 8..10: no window
    assert uniform_windows(4, 4).tolist() == [[0, 1, 2, 3]] and uniform_windows(3, 4).tolist() == [[0, 1, 2, 0]]
    assert uniform_windows(60, 20).shape == (10, 20)
    assert uniform_windows(30, 4, stride=8)[:, 0].tolist() == [0, 8, 16, 24]


# ------------------------------------------------------------------ the pooled item
def _video(f, s=8, p=21, seed=0):
    return torch.randint(0, 256, (f, s, s, p), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_pooled_item_round_trips_and_missing_frames_become_127():
    frames = _video(25)
    missing = {5, 14}
    calls = []

    def read(i):
        calls.append(i)
        return None if i in missing else frames[i]
    win = uniform_windows(25, 4)                                              # starts 0, 4, .., 20: frame 24 unreferenced
    item = make_pooled_item("CropLHand", win, 3, read)
    assert sorted(item) == ["CropLHand_pool", "label", "windows"] and item["label"] == 3
    assert calls == list(range(24))                                           # once each, referenced frames only
    pool, local = item["CropLHand_pool"], item["windows"]
    assert pool.dtype == torch.uint8 and tuple(pool.shape) == (22, 8, 8, 21) and local.dtype == torch.int32
    assert local.shape == win.shape and sorted(set(local.flatten().tolist())) == [-1] + list(range(22))    # dense
    assert (local == -1).sum() == 2 and local[1, 1] == -1 and local[3, 2] == -1
    clips = unpool_item(item)
    assert len(clips) == 6 and all(sorted(c) == ["CropLHand_u8", "label"] and c["label"] == 3 for c in clips)
    want = frames.clone()
    want[sorted(missing)] = 127
    for k, c in enumerate(clips):
        assert torch.equal(c["CropLHand_u8"], want[win[k].long()])
    assert int(clips[1]["CropLHand_u8"][1].min()) == int(clips[1]["CropLHand_u8"][1].max()) == 127
    bad = dict(item, windows=local.clone())
    bad["windows"][0, 0] = 22
    with pytest.raises(ValueError):
        unpool_item(bad)


# ------------------------------------------------------------------ FramePool on the emulated backend
def test_frame_pool_uploads_every_frame_once_across_straddling_batches():
    be = EmuPoolBackend()
    pre = DevicePreprocess("cpu", be)
    T, bs = 4, 3
    videos = [_video(f, seed=i) for i, f in enumerate((3, 11, 25))]
    items = [make_pooled_item("k", uniform_windows(len(v), T), i, v.__getitem__) for i, v in enumerate(videos)]
    items[2]["windows"][2, 1] = -1                                            # a missing frame
    pool = FramePool("cpu", be)
    refs, got, want = [], [], []
    for it in items:                                                          # K = 1, 2, 6: nine windows, batches of three
        base = pool.add(it["k_pool"], it["windows"])
        video = {"base": base, "rows": pool.rows(base, it["windows"]), "left": len(it["windows"])}
        refs += [(video, r) for r in range(video["left"])]
        want += [c["k_u8"] for c in unpool_item(it)]
    assert [v["left"] for v, r in refs if r == 0] == [1, 2, 6]
    while refs:
        batch, refs = refs[:bs], refs[bs:]                                    # the 25-frame video straddles all three
        got.append(pool.gather(torch.stack([v["rows"][r] for v, r in batch])))
        for v, _ in batch:
            v["left"] -= 1
            if v["left"] == 0:
                pool.release(v["base"])
    assert not pool.live
    assert pool.bytes_uploaded == sum(it["k_pool"].numel() for it in items) == (3 + 8 + 24) * 8 * 8 * 21
    got = torch.cat(got)
    assert got.dtype == torch.float32 and tuple(got.shape) == (9, T, 21, 8, 8)
    assert torch.equal(got, pre(torch.stack(want)))
    assert torch.equal(got[5, 1], torch.full((21, 8, 8), float(normalize_lut()[127])))


def test_frame_pool_reuses_released_slots_and_keeps_straddlers_when_it_grows():
    be = EmuPoolBackend()
    pool = FramePool("cpu", be)
    a, b, c = _video(4, seed=1), _video(6, seed=2), _video(3, seed=3)
    ba = pool.add(a)
    bb = pool.add(b)                                                          # grows: a is carried over device to device
    assert (ba, bb) == (0, 4) and pool.bytes_uploaded == (4 + 6) * 8 * 8 * 21
    pool.release(ba)
    bc = pool.add(c)                                                          # first fit: the gap a left
    assert bc == 0 and pool.live == {0: 3, 4: 6}
    lut = normalize_lut()
    got = pool.gather(torch.tensor([[4, 9, 0, 2]], dtype=torch.int32), torch.bfloat16, 5, 15)
    want = lut[torch.stack([b[0], b[5], c[0], c[2]])[None].long()].permute(0, 1, 4, 2, 3)[:, :, 5:20]
    assert got.dtype == torch.bfloat16 and torch.equal(got, want.to(torch.bfloat16))
    with pytest.raises(ValueError):
        pool.gather(torch.tensor([[3]], dtype=torch.int32))                   # a free slot
    with pytest.raises(ValueError):
        pool.gather(torch.tensor([[10]], dtype=torch.int32))
    with pytest.raises(ValueError):
        pool.gather(torch.tensor([[-2]], dtype=torch.int32))


def test_frame_pool_rejects_an_index_outside_its_pool_before_any_upload():
    pool = FramePool("cpu", EmuPoolBackend())
    for bad in (11, -2):
        w = uniform_windows(11, 4)
        w[1, 2] = bad
        with pytest.raises(ValueError):
            pool.add(_video(11), w)
    assert pool.bytes_uploaded == 0 and not pool.live and pool.arena is None
    base = pool.add(_video(11), uniform_windows(11, 4))
    with pytest.raises(ValueError):
        pool.rows(base, torch.tensor([[0, 1, 2, 11]], dtype=torch.int32))


# ------------------------------------------------------------------ Trainer.run_eval
def _cfg(bs, root="/nonexistent"):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "slowfast-LHand"
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.DEPTH = 18
    cfg.NUM_CPU = 0
    return cfg


class _Unpooled(torch.utils.data.Dataset):
    def __init__(self, pooled_set):
        self.s = pooled_set

    def __len__(self):
        return len(self.s)

    def __getitem__(self, i):
        return unpool_item(self.s[i])


def test_synthetic_chalearn_pooled_items():
    cfg = _cfg(2)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=5, seed=2, pooled=True, frames_per_video=(3, 14))
    plain = v1.SyntheticChalearn(cfg, "test", num_videos=5, seed=2)
    assert te.labels == plain.labels and all(3 <= f <= 14 for f in te.nframes) and len(set(te.nframes)) > 1
    for i in range(5):
        it = te[i]
        assert sorted(it) == ["CropLHand_pool", "label", "windows"] and it["label"] == te.labels[i]
        win = uniform_windows(te.nframes[i], 4)
        assert te.nclips[i] == win.shape[0] == it["windows"].shape[0] and it["windows"].dtype == torch.int32
        assert tuple(it["CropLHand_pool"].shape) == (len(set(win.flatten().tolist())), 64, 64, 21)
        assert torch.equal(it["CropLHand_pool"], te[i]["CropLHand_pool"])
    # without the flag: the items and the draws behind them are what they were
    again = v1.SyntheticChalearn(cfg, "test", num_videos=5, seed=2, pooled=False)
    assert again.nclips == plain.nclips and torch.equal(again[1][0]["CropLHand"], plain[1][0]["CropLHand"])
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=2, pooled=True)
    assert "CropLHand" in tr[0]                                               # train items are never pooled


@pytest.mark.parametrize("bs", [2, 5])
def test_run_eval_pooled_equals_run_eval_on_the_unpooled_videos(bs):
    cfg = _cfg(bs)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=4, seed=2, pooled=True, frames_per_video=(3, 14))
    assert sum(te.nclips) > bs and max(te.nclips) >= 2
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuPoolBackend())
    flat = torch.utils.data.DataLoader(_Unpooled(te), batch_size=bs, shuffle=False, collate_fn=lambda x: x)
    a, b = t.run_eval(flat), t.run_eval(flat)
    spread = float(np.abs(a["ps"] - b["ps"]).max())                           # run to run, unpooled
    assert getattr(t, "frame_pool", None) is None                             # lists never touch the pool
    got = t.run_eval()
    assert got["sv"] == a["sv"] == te.nclips
    assert np.array_equal(got["t"], a["t"]) and got["acc"] == a["acc"]
    err = float(np.abs(got["ps"] - a["ps"]).max())
    print(f"pooled run_eval bs {bs}: |ps - unpooled| {err:.3e}, unpooled run-to-run {spread:.3e}")
    assert err <= spread
    assert t.frame_pool.bytes_uploaded == sum(te[i]["CropLHand_pool"].numel() for i in range(len(te))) and not t.frame_pool.live
    t.run_eval()
    assert t.frame_pool.bytes_uploaded == sum(te[i]["CropLHand_pool"].numel() for i in range(len(te)))   # per run_eval


def test_pooled_eval_ignores_u8_stem():
    """MODEL.U8_STEM: true does not change the pooled path: the stems get the gathered float clip"""
    res = []
    for on in (False, True):
        cfg = _cfg(2)
        cfg.MODEL.U8_STEM = on
        tr = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
        te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=3, pooled=True, frames_per_video=(5, 9))
        torch.manual_seed(0)
        t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuPoolBackend())
        seen = []
        prepare = t.mm.prepare_data
        t.mm.prepare_data = lambda batch: (seen.append(sorted(batch)), prepare(batch))[1]
        res.append(t.run_eval()["ps"])
        assert all(k == ["CropLHand", "label"] for k in seen)
    assert np.array_equal(res[0], res[1])


# ------------------------------------------------------------------ the frames loader
def _tree(tmp_path, videos, missing=()):
    """ROOT/2_Images/<set>/001/M_0000i/000kk.jpg name the frames; ROOT/CropLHand/... holds those that 'exist'"""
    cfg = _cfg(2, tmp_path)
    labels = []
    for i, f in enumerate(videos):
        rel = f"test/001/M_{i:05d}"
        (tmp_path / "2_Images" / rel).mkdir(parents=True)
        (tmp_path / "CropLHand" / rel).mkdir(parents=True)
        for k in range(f):
            (tmp_path / "2_Images" / rel / f"{k * 5:05d}.jpg").write_bytes(b"")
            if (i, k) not in missing:
                (tmp_path / "CropLHand" / rel / f"{k * 5:05d}.jpg").write_bytes(b"")
        labels.append((rel + ".avi", rel.replace("M_", "K_") + ".avi", i + 1))
    calls = []

    def read_frame(path, size):
        calls.append(str(path))
        if not os.path.exists(path):
            return None
        k = int(os.path.basename(path)[:5]) // 5
        return np.full((size, size, 21), k, dtype=np.uint8)
    return cfg, labels, read_frame, calls


def test_chalearn_video_frames_u8(tmp_path):
    cfg, labels, read_frame, calls = _tree(tmp_path, [11, 3], missing={(0, 5)})
    ds = v1.ChalearnVideoFramesU8(cfg, "test", labels, read_frame)
    assert len(ds) == 2
    it = ds[0]                                                                # 11 frames, T 4: windows at 0 and 4
    assert len(calls) == len(set(calls)) == 8 and all("/CropLHand/test/001/M_00000/" in c for c in calls)
    assert sorted(it) == ["CropLHand_pool", "label", "windows"] and it["label"] == 0
    assert it["windows"].tolist() == [[0, 1, 2, 3], [4, -1, 5, 6]]            # frame 5 has no file
    assert tuple(it["CropLHand_pool"].shape) == (7, 64, 64, 21) and it["CropLHand_pool"][:, 0, 0, 0].tolist() == [0, 1, 2, 3, 4, 6, 7]
    del calls[:]
    it = ds[1]                                                                # 3 frames: one wrapped window
    assert len(calls) == 3 and it["windows"].tolist() == [[0, 1, 2, 0]] and it["label"] == 1
    flat = v1.ChalearnVideoFramesU8(cfg, "valid", labels, read_frame, pooled=False)[0]
    assert isinstance(flat, list) and len(flat) == 2 and sorted(flat[1]) == ["CropLHand_u8", "label"]
    assert flat[1]["CropLHand_u8"][:, 3, 3, 20].tolist() == [4, 127, 6, 7]
    cfg.MODEL.COLOR_JITTER = True
    tr = v1.ChalearnVideoFramesU8(cfg, "train", labels, read_frame)[0]
    assert sorted(tr) == ["CropLHand_u8", "crop", "jitter", "label"] and tr["label"] == 0
    assert tr["CropLHand_u8"].dtype == torch.uint8 and tuple(tr["CropLHand_u8"].shape) == (4, 64, 64, 21)
    assert tr["crop"].dtype == torch.int32 and tuple(tr["crop"].shape) == (2,) and tuple(tr["jitter"].shape) == (8,)
    first = tr["CropLHand_u8"][:, 0, 0, 0].tolist()                           # a random start in 0..7; frame 5 has no file
    assert first[0] in (0, 1, 2, 3, 4, 127, 6, 7)
    # every start random_sampling can draw (randint(0, seq_len - clip_len), both ends included), and the wrapped short video
    class Fixed:
        def __init__(self, start):
            self.start, self.asked = start, []

        def randint(self, lo, hi):
            self.asked.append((lo, hi))
            return self.start
    ds_tr = v1.ChalearnVideoFramesU8(cfg, "train", labels, read_frame)
    for start in range(8):
        ds_tr.rng = Fixed(start)
        got = ds_tr[0]["CropLHand_u8"]
        assert ds_tr.rng.asked == [(0, 7)]
        assert got[:, 0, 0, 0].tolist() == [127 if k == 5 else k for k in range(start, start + 4)], start
        assert all(int(f.min()) == int(f.max()) for f in got)                 # whole frames, the missing one 127 everywhere
    ds_tr.rng = Fixed(0)
    assert ds_tr[1]["CropLHand_u8"][:, 0, 0, 0].tolist() == [0, 1, 2, 0] and ds_tr.rng.asked == [(0, 0)]
    cfg.MODEL.COLOR_JITTER = False
    assert "jitter" not in v1.ChalearnVideoFramesU8(cfg, "train", labels, read_frame)[1]
    assert "jitter" not in ds[0]


def test_chalearn_video_frames_u8_feeds_run_eval(tmp_path):
    cfg, labels, read_frame, calls = _tree(tmp_path, [11, 3, 9], missing={(2, 1)})
    te = v1.ChalearnVideoFramesU8(cfg, "test", labels, read_frame)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuPoolBackend())
    res = t.run_eval()
    assert res["sv"] == [2, 1, 2] and res["t"].tolist() == [0, 0, 1, 2, 2] and res["ps"].shape == (5, 7)
    assert t.frame_pool.bytes_uploaded == (8 + 3 + 7) * 64 * 64 * 21


def test_default_reader_needs_cv2_and_says_so(tmp_path):
    try:
        import cv2  # noqa: F401
    except Exception:
        with pytest.raises(RuntimeError, match="cv2"):
            v1.cv2_read_frame(tmp_path / "00000.jpg", 64)
    else:
        assert v1.cv2_read_frame(tmp_path / "00000.jpg", 64) is None
