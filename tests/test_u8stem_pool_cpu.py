"""MODEL.POOL_STEM on CPU: the uint8 stems reading the frame pool through its index table (include/sfk_u8stem_pool.h,
input_pipeline.PoolClip, FramePool.clip), emulated by tests/emu_u8stem_pool.py.  The virtual clip against the stacked-frame
U8Clip's, the ctypes binding of the new header and its host-side rejections, the Trainer on the resident set and the pooled
run_eval with the switch on and off (exact under emulation, no gather, no float clip, the same uploads and arena
bookkeeping), the addresses equal-shaped batches hand the stems, and the combinations the switch refuses."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emu_u8stem
from emu_u8stem_pool import EmuU8StemPoolBackend, materialize
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import FramePool, PoolClip, ResidentTrainSet, U8Clip, normalize_lut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "CropLHand"                                                               # 64 x 64 crops
FRAME = 64 * 64 * 21


# ------------------------------------------------------------------ the virtual clip
@pytest.mark.parametrize("pitch,c0,c", [(21, 0, 5), (21, 5, 15), (21, 5, 5), (5, 0, 5)])
@pytest.mark.parametrize("crop", [None, [[0, 2], [3, 0], [1, 1]], [[-40, 1], [2, 2 ** 31 - 1], [2, 0]]])
def test_pool_clip_is_the_u8_clip_of_the_stacked_frames(pitch, c0, c, crop):
    """shuffled, repeated, -1 and >= frames indices; with and without a crop; c0 0 and 5; pitch 21 and 5"""
    g = torch.Generator().manual_seed(pitch + c0)
    f, s, pad, fill = 7, 12, 1, 127
    arena = torch.randint(0, 256, (f, s, s, pitch), generator=g, dtype=torch.uint8)
    index = torch.tensor([[5, 0, 3, 3], [3, -1, 6, f], [0, 1, 2, 2 ** 31 - 1]], dtype=torch.int32)
    crop = None if crop is None else torch.tensor(crop, dtype=torch.int32)
    lut = normalize_lut()
    ext = torch.cat([arena, torch.full((1, s, s, pitch), fill, dtype=torch.uint8)])          # the last frame stands for "missing"
    idx = index.long()
    stacked = ext[torch.where((idx < 0) | (idx >= f), torch.full_like(idx, f), idx)]         # (n, t, s, s, pitch)
    want = emu_u8stem.materialize(U8Clip(stacked, c0, c, crop, pad, lut))
    x = PoolClip(arena, index, c0, c, crop, pad, lut, fill)
    got = materialize(x)
    assert tuple(got.shape) == tuple(x.shape) == (3, c, 4, s, s) and torch.equal(got, want)
    assert (x.dim(), x.dtype, x.numel(), x.element_size()) == (5, torch.uint8, 3 * c * 4 * s * s, 1)
    assert x.geometry_key() != U8Clip(stacked, c0, c, crop, pad, lut).geometry_key()


# ------------------------------------------------------------------ the binding of include/sfk_u8stem_pool.h
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def test_u8stem_pool_table_matches_its_header(lib):
    from video_classification_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfk_u8stem_pool.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_U8STEM_POOL) == ["sfk_u8pstem2d_fwd", "sfk_u8pstem2d_wgrad", "sfk_u8pstem_conv_fwd",
                                                            "sfk_u8pstem_conv_wgrad", "sfk_u8stem_pool_abi_version"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STEM2D, _lib.SIGNATURES_U8STEM, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG,
                  _lib.SIGNATURES_POOL, _lib.SIGNATURES_RESIZE, _lib.SIGNATURES_RESIDENT, _lib.SIGNATURES_ROI_POOL,
                  _lib.SIGNATURES_ROI_RAGGED):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None          # exported and bound
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_U8STEM_POOL[n]), n
        # the signature of the stacked-frame counterpart, with the new descriptor in place of sfk_u8_clip
        twin = n.replace("u8pstem", "u8stem")
        if twin != n:
            assert [a for a in _lib.SIGNATURES_U8STEM_POOL[n][1:]] == [a for a in _lib.SIGNATURES_U8STEM[twin][1:]]
    assert lib.sfk_u8stem_pool_abi_version() == _lib.U8STEM_POOL_ABI_VERSION == 1 == int(
        re.search(r"#define\s+SFK_U8STEM_POOL_ABI_VERSION\s+(\d+)", src).group(1))
    body = re.search(r"typedef struct \{(.*?)\} sfk_u8_pool_clip;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            fields += [nm.strip() for nm in m.group(3).replace("*", "").split(",")]
    assert [f for f, _ in _lib._U8PoolClip._fields_] == fields
    assert [f for f in fields if f != "reserved0"] == ["struct_size", "pool", "frame_stride", "row_stride", "pixel_pitch", "frames",
                                                       "c0", "c", "n", "t", "h", "w", "index", "lut", "crop", "pad", "fill"]


def test_u8_pool_clip_size_is_what_gcc_says(tmp_path):
    from video_classification_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_u8stem_pool.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(sfk_u8_pool_clip), '
                                  'offsetof(sfk_u8_pool_clip, pool), offsetof(sfk_u8_pool_clip, index), '
                                  'offsetof(sfk_u8_pool_clip, crop), offsetof(sfk_u8_pool_clip, fill)); return 0; }\n')
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    got = tuple(int(v) for v in subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split())
    D = _lib._U8PoolClip
    assert got == (ctypes.sizeof(D), D.pool.offset, D.index.offset, D.crop.offset, D.fill.offset)
    assert got[0] == 96 == _lib.new_u8_pool_clip().struct_size


def test_u8stem_pool_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test): the cases of sfk_u8stem_* and those of
    sfk_u8_pool_gather_crop, through all four entry points"""
    from video_classification_amd import _lib
    buf = torch.zeros(1024, dtype=torch.float32)
    before = buf.clone()
    lut = torch.zeros(256, dtype=torch.float32)
    pool = torch.zeros(3 * 64 * 64 * 21, dtype=torch.uint8)
    index, crop = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32)

    def good():
        d = _lib.new_u8_pool_clip()
        d.pool, d.index, d.lut, d.crop, d.pad, d.fill = pool.data_ptr(), index.data_ptr(), lut.data_ptr(), crop.data_ptr(), 6, 127
        d.frame_stride, d.row_stride, d.pixel_pitch, d.frames = 64 * 64 * 21, 64 * 21, 21, 3
        d.c0, d.c, d.n, d.t, d.h, d.w = 0, 5, 2, 2, 64, 64
        return d

    def fmap(t):
        y = _lib._FMap()
        y.ptr, y.dtype = buf.data_ptr(), _lib.SFK_F32
        y.n, y.t, y.h, y.w, y.c, y.ld, y.c_off = 2, t, 32, 32, 64, 64, 0
        return y

    B = ctypes.byref
    y3, y2, p = fmap(2), fmap(1), buf.data_ptr()

    def calls(d, y3=y3, y2=y2, w=p, kt=1):
        return [lib.sfk_u8pstem_conv_fwd(B(d), None, 0, kt, w, B(y3), None, None),
                lib.sfk_u8pstem_conv_wgrad(B(d), None, 0, kt, B(y3), w, None),
                lib.sfk_u8pstem2d_fwd(B(d), w, B(y2), None, None),
                lib.sfk_u8pstem2d_wgrad(B(d), B(y2), w, None)]

    for field, value in [("struct_size", 8), ("struct_size", 88), ("struct_size", 104), ("pool", None), ("index", None),
                         ("lut", None), ("pad", -1), ("c0", -1), ("c0", 17), ("c", 22), ("c", 0), ("pixel_pitch", 4), ("n", 0),
                         ("t", 0), ("h", -4), ("w", 0), ("frames", 0), ("frames", -3), ("frame_stride", -1),
                         ("row_stride", -1), ("fill", -1), ("fill", 256)]:
        d = good()
        setattr(d, field, value)
        assert calls(d) == [-1] * 4, (field, value)
    assert calls(good(), w=None) == [-1] * 4                                                   # a NULL filter / dw
    assert calls(good(), kt=2)[:2] == [-1] * 2                                                 # an even kt (3-D only)
    assert lib.sfk_u8pstem_conv_fwd(None, None, 0, 1, p, B(y3), None, None) == -1
    assert lib.sfk_u8pstem2d_wgrad(None, B(y2), p, None) == -1
    d = good()
    d.crop = None                                                                              # no crop: still a good descriptor,
    d.c0, d.c, d.pixel_pitch = 5, 15, 20                                                       # c0 + c == pitch: accepted
    y3.c = y2.c = 62                                                                           # ... up to cout % 4
    assert calls(d) == [-2] * 4
    y3.c = y2.c = y3.ld = y2.ld = 128                                                          # cout > 64
    assert calls(d) == [-2] * 4
    y3.c = y2.c = y3.ld = y2.ld = 64
    assert lib.sfk_u8pstem_conv_fwd(B(good()), None, 0, 1, p + 4, B(y3), None, None) == -2      # a misaligned filter
    assert lib.sfk_u8pstem2d_fwd(B(good()), p + 4, B(y2), None, None) == -2
    # the map's clip count must be the descriptor's: tiles index clips, table rows and crop rows by it
    y3.n = y2.n = 3
    assert calls(good()) == [-1] * 4
    assert torch.equal(buf, before)


# ------------------------------------------------------------------ FramePool.clip
def test_frame_pool_clip_checks_like_gather_and_keeps_its_addresses():
    be = EmuU8StemPoolBackend()
    pool = FramePool("cpu", be, capacity=12)
    g = torch.Generator().manual_seed(0)
    a = pool.add(torch.randint(0, 256, (5, 20, 20, 21), generator=g, dtype=torch.uint8))
    b = pool.add(torch.randint(0, 256, (4, 20, 20, 21), generator=g, dtype=torch.uint8))
    rows = torch.tensor([[a, a + 4, -1], [b + 3, b, a + 2]], dtype=torch.int32)
    crop = torch.tensor([[0, 4], [3, 1]], dtype=torch.int32)
    slow, fast = pool.clip(rows, [(0, 5), (5, 15)], crop=crop)
    assert be.calls == [] and (slow.c0, slow.c, fast.c0, fast.c, slow.pad, slow.fill) == (0, 5, 5, 15, 2, 127)
    assert slow.arena is pool.arena and slow.index is fast.index and slow.crop is fast.crop
    want = pool.gather(rows, crop=crop)                                                  # (n, t, 21, h, w)
    assert torch.equal(materialize(slow), want.permute(0, 2, 1, 3, 4)[:, 0:5])
    assert torch.equal(materialize(fast), want.permute(0, 2, 1, 3, 4)[:, 5:20])
    ptrs = slow.bound_ptrs()
    again = pool.clip(torch.tensor([[b, b, b], [-1, a, a + 1]], dtype=torch.int32), [(0, 5)], crop=crop.flip(0))[0]
    assert again.bound_ptrs() == ptrs and again.geometry_key() == slow.geometry_key()
    assert slow.index.tolist() == [[b, b, b], [-1, a, a + 1]]                             # the SAME tables, overwritten
    small = pool.clip(torch.tensor([[a, a, a]], dtype=torch.int32), [(0, 5)], crop=crop[:1])[0]
    assert small.bound_ptrs() == ptrs and small.geometry_key() != slow.geometry_key()     # a smaller batch: the same base
    test_clip = pool.clip(rows, [(0, 5)])[0]                                              # no crop (eval)
    assert test_clip.crop is None and torch.equal(materialize(test_clip), pool.gather(rows).permute(0, 2, 1, 3, 4)[:, 0:5])
    with pytest.raises(ValueError, match="^clip: an index is neither -1 nor a slot"):      # (the error names its caller)
        pool.clip(torch.tensor([[a, 9, -1]], dtype=torch.int32), [(0, 5)])                # slot 9 belongs to no video
    with pytest.raises(ValueError, match="^gather: an index is neither -1 nor a slot"):
        pool.gather(torch.tensor([[a, 9, -1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="neither -1 nor a slot"):
        pool.clip(torch.tensor([[-2, a, a]], dtype=torch.int32), [(0, 5)])
    pool.release(b)
    with pytest.raises(ValueError, match="neither -1 nor a slot"):
        pool.clip(rows, [(0, 5)])


# ------------------------------------------------------------------ the Trainer switch
def _cfg(name, on, bs=2, jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = KEY
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 24 * FRAME / 2 ** 30                                  # 24 slots: 16 resident + the spill region of 8
    cfg.MODEL.POOL_STEM = on
    cfg.MODEL.LR = 1e-3
    cfg.NUM_CPU = 0
    return cfg


def _sets(cfg):
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True, frames_per_video=(3, 8))
    te = v1.SyntheticChalearn(cfg, "test", num_videos=3, seed=2, pooled=True, frames_per_video=(3, 9))
    return tr, te


def test_config_default_is_off():
    from video_classification_amd.config import get_cfg
    assert get_cfg().MODEL.POOL_STEM is False


def _run(name, on):
    cfg = _cfg(name, on)
    tr, te = _sets(cfg)
    be = EmuU8StemPoolBackend()
    torch.manual_seed(0)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    assert t.pool_stem is on and isinstance(t.resident, ResidentTrainSet)
    seen, ptrs = [], []
    prepare = t.mm.prepare_data

    def spy(batch):
        seen.append(batch[KEY])
        x, y = prepare(batch)
        clips = [x] if isinstance(x, (torch.Tensor, PoolClip)) else list(x)
        ptrs.append((len(batch["label"]), tuple(c.bound_ptrs() if isinstance(c, PoolClip) else None for c in clips)))
        return x, y
    t.mm.prepare_data = spy
    out = {"loss": [], "spilled": []}
    for epoch in range(2):
        t.epoch = epoch
        out["loss"].append(t.train_epoch()[0])
        out["spilled"].append(t.resident.spilled_clips)
        assert sorted(t.resident.pool.live) == sorted(set(t.resident.pool.live)) and sum(
            t.resident.pool.live.values()) == t.resident.resident_frames              # no spill slot outlives its epoch
    ntrain = len(seen)
    out["ps"] = t.run_eval()["ps"]
    out.update(train_bytes=t.resident.bytes_uploaded, train_live=dict(t.resident.pool.live), eval_bytes=t.frame_pool.bytes_uploaded,
               eval_live=dict(t.frame_pool.live), weights={k: v.clone() for k, v in t.model.state_dict().items()},
               seen=seen, ptrs=ptrs, ntrain=ntrain, calls=list(be.calls), spill_peak=t.resident.spill_peak)
    return out


@pytest.mark.parametrize("name", ["res3d", "res2d", "slowfast-LHand"])
def test_trainer_pool_stem_on_and_off_agree_exactly(name):
    off, on = _run(name, False), _run(name, True)
    assert off["spilled"] == on["spilled"] and sum(off["spilled"]) > 0 and off["spill_peak"] == on["spill_peak"] > 0
    assert off["loss"] == on["loss"] and np.array_equal(off["ps"], on["ps"])
    assert all(torch.equal(off["weights"][k], on["weights"][k]) for k in off["weights"])
    # off: the float clip of one gather per batch; on: PoolClips, and no gather at all
    assert len(off["seen"]) == len(on["seen"]) > off["ntrain"] == on["ntrain"] == 4
    assert all(torch.is_tensor(x) and x.dtype == torch.float32 for x in off["seen"])
    assert off["calls"].count("u8_pool_gather_crop") == 4 and off["calls"].count("u8_pool_gather") == len(off["seen"]) - 4
    assert on["calls"] == []
    npath = 2 if name.startswith("slowfast") else 1
    for x in on["seen"]:
        assert isinstance(x, list) and len(x) == npath and all(isinstance(c, PoolClip) for c in x)
        assert [(c.c0, c.c) for c in x] == [(0, 5), (5, 15)][:npath]
    assert all(x[0].crop is not None for x in on["seen"][:4]) and all(x[0].crop is None for x in on["seen"][4:])
    # the uploads and the arenas' bookkeeping are those of the gathered route
    assert (off["train_bytes"], off["eval_bytes"]) == (on["train_bytes"], on["eval_bytes"])
    assert off["train_live"] == on["train_live"] and off["eval_live"] == on["eval_live"] == {}
    # equal-shaped batches of an epoch (all four train batches: the arena has a fixed capacity) hand the stems the same addresses
    train = on["ptrs"][:4]
    assert all(p == train[0] for p in train) and all(q is not None for q in train[0][1])
    assert all(q is None for _, qs in off["ptrs"] for q in qs)


def _resident(on, be=None):
    cfg = _cfg("res3d", on)
    tr, _ = _sets(cfg)
    return ResidentTrainSet(tr, cfg, "cpu", be or EmuU8StemPoolBackend(), batch_size=2,
                            stem_channels=[(0, 5)] if on else None)


@pytest.mark.parametrize("how", ["break", "raise", "drop"])
def test_an_epoch_left_early_gives_its_spill_slots_back(how):
    """the consumer stops inside a batch that has spilled clips -- a break (DEBUG), an exception in its step, the generator
    dropped: the arena's bookkeeping is the gathered route's, epoch after epoch"""
    live = []
    for on in (False, True):
        r = _resident(on)
        seen = []
        for epoch in range(8):
            it = r.epoch(epoch)
            try:
                for k, batch in enumerate(it):
                    spilled = r.spilled_clips
                    if how == "raise" and k == 1:
                        raise KeyError("the step failed")
                    if k == 1:
                        break
            except KeyError:
                pass
            if how != "drop":
                it.close()
            del it                                                            # (dropped: CPython closes it here)
            seen.append((spilled, dict(r.pool.live)))
        assert any(s > 0 for s, _ in seen)                                    # batches with spilled clips were left early
        assert all(sum(lv.values()) == r.resident_frames for _, lv in seen)   # nothing but the resident videos stays
        live.append(seen)
    assert live[0] == live[1]


def test_debug_trainer_does_not_fill_the_arena():
    """cfg.DEBUG breaks out of every train epoch after one batch: the arena holds what the gathered route's holds"""
    live = []
    for on in (False, True):
        cfg = _cfg("res3d", on)
        cfg.DEBUG = True
        tr, te = _sets(cfg)
        torch.manual_seed(0)
        t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuU8StemPoolBackend())
        one = []
        for epoch in range(8):
            t.epoch = epoch
            t.train_epoch()
            one.append(dict(t.resident.pool.live))
        live.append(one)
    assert live[0] == live[1] and max(sum(lv.values()) for lv in live[1]) <= 16    # the resident region, never a spill slot


def test_pool_stem_refuses_what_it_cannot_do(monkeypatch):
    from video_classification_amd import gesture_v2 as v2
    be = EmuU8StemPoolBackend()
    cfg = _cfg("slowfast-LHand", True, jitter=True)
    tr, te = _sets(cfg)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    with pytest.raises(ValueError, match="POOL_STEM.*no float clip.*COLOR_JITTER"):       # U8_STEM's refusal, word for word
        t.train_epoch()
    u8 = _cfg("slowfast-LHand", False, jitter=True)
    u8.MODEL.RESIDENT_TRAIN, u8.MODEL.U8_STEM = False, True
    with pytest.raises(ValueError, match="U8_STEM.*no float clip.*COLOR_JITTER"):
        v1.Trainer(u8, train_set=tr, test_set=te, device="cpu", backend=be).train_epoch()
    monkeypatch.setattr(v1.sdist, "init_process_group_from_env", lambda backend=None: (0, 2, None))
    with pytest.raises(ValueError, match="POOL_STEM.*WORLD_SIZE"):
        v1.Trainer(_cfg("slowfast-LHand", True), train_set=tr, test_set=te, device="cpu", backend=be)
    monkeypatch.undo()
    res2d = _cfg("res2d", True)
    res2d.MODEL.RES2D_BACKEND = "torch"
    res2d.MODEL.RESIDENT_TRAIN = False
    with pytest.raises(ValueError, match="POOL_STEM.*res2d.*torch"):
        v1.Trainer(res2d, train_set=tr, test_set=te, device="cpu", backend=be)
    g = _cfg("gesture-v2", True)
    g.MODEL.RESIDENT_TRAIN = False
    g.MODEL.INPUT_SIZE = 64
    gtr = v2.SyntheticGesture(g, "train", num_videos=2, seed=1, h=48, w=64, min_box=8)
    gte = v2.SyntheticGesture(g, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    with pytest.raises(ValueError, match="POOL_STEM.*part-box.*BEFORE the stem"):
        v2.Trainer(g, train_set=gtr, test_set=gte, device="cpu", backend=be)
    # off: none of these is refused for the switch's sake
    g.MODEL.POOL_STEM = False
    assert v2.Trainer(g, train_set=gtr, test_set=gte, device="cpu", backend=be).pool_stem is False


def test_pool_stem_without_the_resident_set_only_changes_pooled_eval():
    """MODEL.POOL_STEM with RESIDENT_TRAIN off: the train loader's uint8 batches go the way they went (jitter included); the
    pooled run_eval reads the pool in the stems"""
    ps = []
    for on in (False, True):
        cfg = _cfg("res3d", on, jitter=True)
        cfg.MODEL.RESIDENT_TRAIN = False
        tr, te = _sets(cfg)
        be = EmuU8StemPoolBackend()
        torch.manual_seed(0)
        t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
        assert not hasattr(t, "resident")
        seen = []
        prepare = t.mm.prepare_data
        t.mm.prepare_data = lambda batch: (seen.append(sorted(batch)), prepare(batch))[1]
        torch.manual_seed(1)
        t.train_epoch()
        assert seen == [[KEY + "_u8", "crop", "jitter", "label"]] * 2
        ps.append(t.run_eval()["ps"])
        assert (be.calls == []) is on and not t.frame_pool.live
    assert np.array_equal(ps[0], ps[1])
