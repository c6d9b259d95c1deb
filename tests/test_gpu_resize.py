"""sfk_u8_pad_resize_cubic on an MI355X (include/sfk_resize.h) against tests/ref_resize.py: bit-exact frames for up- and
downscales, odd padding, the identity, one-pixel sources and clamped overshoot, with never-aligned (S = 13) and aligned (S = 16)
output rows and 21 or 5 channels; the float64 cubic within one grey level; missing frames and untouched memory around strided
output slots; a frame beyond byte 2^31; reproducibility; a captured graph following new table contents and bytes; the host-side
rejections; a launch sized for 640-pixel sources (more than 64 KB of LDS); FramePool.add_raw; Trainer.run_eval on raw pooled
videos and prepare_data on raw train batches.  The arithmetic is integer on both sides, so every comparison is torch.equal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ref_resize
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import (MISSING_BYTE, FramePool, PadResize, collate_raw, make_raw_pooled_item,
                                                     pack_raw_frames, raw_offsets, uniform_windows)

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (h, w): upscale with odd padding, wide, the identity at S 16, downscale, a 4x downscale whose taps skip pixels, one pixel, two rows
SHAPES = [(5, 3), (9, 16), (16, 16), (37, 23), (40, 64), (1, 1), (2, 7)]
BINARY = (12, 9)                                                              # a 0/255 frame: its overshoot clamps at both ends


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def case(c, size):
    """the frames of one launch, their packed bytes and table, and the reference's answer (computed once, never changed)"""
    g = torch.Generator().manual_seed(1000 * c + size)
    frames = [torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8) for h, w in SHAPES]
    frames.append((torch.randint(0, 2, BINARY + (c,), generator=g) * 255).to(torch.uint8))
    raw, hw = pack_raw_frames(frames)
    offset = raw_offsets(hw, c)
    want = torch.from_numpy(ref_resize.resize_table(raw.numpy(), offset.numpy(), hw.numpy(), c, size, 64, 127))
    want.requires_grad_(False)
    return frames, raw, offset, hw, want


def launch(hip, raw_dev, offset, hw, c, size, max_side=64, fill=127, out=None):
    if out is None:
        out = torch.full((hw.shape[0], size, size, c), 77, dtype=torch.uint8, device=DEV)
    hip.u8_pad_resize_cubic(raw_dev, offset.to(DEV), hw.to(DEV), out, size, max_side, fill)(stream())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("size", [16, 13])
@pytest.mark.parametrize("c", [21, 5])
def test_frames_are_bit_exact(hip, c, size):
    frames, raw, offset, hw, want = case(c, size)
    got = launch(hip, raw.to(DEV), offset, hw, c, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(frames), size, size, c)
    for i, f in enumerate(frames):
        assert torch.equal(got[i], want[i]), (i, tuple(f.shape))
    if size == 16:                                                            # m == S: the zero-padded source itself
        assert torch.equal(got[2], frames[2]) and np.array_equal(got[2].numpy(), ref_resize.pad_square(frames[2].numpy()))
    # the 0/255 frame: the reference holds both 0 and 255 where the unclamped value is outside 0..255
    r = ref_resize.pad_resize_int(frames[-1].numpy(), size, unclamped=True)
    w = want[-1].numpy()
    assert int(r.min()) < 0 and int(r.max()) > 255 and bool((w[r < 0] == 0).all()) and bool((w[r > 255] == 255).all())


@pytest.mark.parametrize("size", [16, 13])
@pytest.mark.parametrize("c", [21, 5])
def test_frames_are_within_one_of_the_float64_cubic(hip, c, size):
    frames, raw, offset, hw, _ = case(c, size)
    got = launch(hip, raw.to(DEV), offset, hw, c, size).numpy().astype(np.int64)
    for i, f in enumerate(frames):
        diff = int(np.abs(got[i] - ref_resize.pad_resize_f64(f.numpy(), size).astype(np.int64)).max())
        print(f"{tuple(f.shape)} -> {size}: max |gpu - f64| {diff}")
        assert diff <= 1, (tuple(f.shape), diff)


@pytest.mark.parametrize("fill", [127, 0])
def test_missing_frames_and_untouched_memory(hip, fill):
    c, size, guard = 5, 13, 48
    frames, raw, offset, hw, want = case(c, size)
    n = len(frames)
    # frame 1: (0, 0); frame 3: its span runs one byte past src_bytes (the buffer is cut there); frame 4: above max_side
    hw2, off2 = hw.clone(), offset.clone()
    hw2[1] = 0
    order = [0, 1, 2, 4, 5, 6, 7, 3]                                          # frame 3's bytes last, so that cutting one cuts its span
    raw2, at = [], 0
    for i in order:
        h, w = hw[i].tolist()
        off2[i] = at
        raw2.append(raw[int(offset[i]):int(offset[i]) + h * w * c])
        at += h * w * c
    raw2 = torch.cat(raw2)[:-1]
    max_side = 39                                                             # frame 4 is (40, 64)
    stride = size * size * c + 37                                             # slots that are not contiguous
    buf = torch.full((guard + n * stride + guard,), 201, dtype=torch.uint8, device=DEV)
    out = buf[guard:guard + n * stride].as_strided((n, size, size, c), (stride, size * c, c, 1))
    got = launch(hip, raw2.to(DEV), off2, hw2, c, size, max_side=max_side, fill=fill, out=out)
    for i in range(n):
        if i in (1, 3, 4):
            assert bool((got[i] == fill).all()), i
        else:
            assert torch.equal(got[i], want[i]), i
    assert torch.equal(got, torch.from_numpy(ref_resize.resize_table(raw2.numpy(), off2.numpy(), hw2.numpy(), c, size, max_side, fill)))
    flat = buf.cpu()
    assert bool((flat[:guard] == 201).all()) and bool((flat[guard + n * stride:] == 201).all())
    gaps = flat[guard:guard + n * stride].view(n, stride)[:, size * size * c:]
    assert bool((gaps == 201).all())                                          # between the slots


def test_a_frame_beyond_byte_2_31(hip):
    c, size = 21, 13
    frames, raw, offset, hw, want = case(c, size)
    far = 2 ** 31 + 1003                                                      # not a multiple of 16 either
    big = torch.empty(far + raw.numel(), dtype=torch.uint8, device=DEV)       # uninitialised: only the frames are written
    big[far:].copy_(raw.to(DEV))
    sel = [3, 0]
    got = launch(hip, big, (offset[sel] + far), hw[sel], c, size)
    assert int(offset[3]) + far > 2 ** 31 and torch.equal(got, want[sel])
    del big
    torch.cuda.empty_cache()


def test_two_launches_give_equal_bytes(hip):
    frames, raw, offset, hw, want = case(21, 16)
    rd = raw.to(DEV)
    a, b = launch(hip, rd, offset, hw, 21, 16), launch(hip, rd, offset, hw, 21, 16)
    assert torch.equal(a, b) and torch.equal(a, want)


def test_sources_of_640_pixels_a_side(hip):
    """max_side 640 with 21 channels asks for more than 64 KB of LDS: the launch opts in, and a 640-pixel row is staged"""
    g = torch.Generator().manual_seed(640)
    frames = [torch.randint(0, 256, (3, 640, 21), generator=g, dtype=torch.uint8), torch.randint(0, 256, (9, 7, 21), generator=g, dtype=torch.uint8)]
    raw, hw = pack_raw_frames(frames)
    offset = raw_offsets(hw, 21)
    got = launch(hip, raw.to(DEV), offset, hw, 21, 16, max_side=640)
    assert torch.equal(got, torch.from_numpy(ref_resize.resize_table(raw.numpy(), offset.numpy(), hw.numpy(), 21, 16, 640, 127)))


def test_captured_graph_follows_new_table_contents_and_bytes(hip):
    c, size = 21, 13
    frames, raw, offset, hw, want = case(c, size)
    sel = [0, 3, 5]
    rd, od, hd = raw.to(DEV), offset[sel].to(DEV), hw[sel].to(DEV)
    out = torch.empty(3, size, size, c, dtype=torch.uint8, device=DEV)
    run = hip.u8_pad_resize_cubic(rd, od, hd, out, size, 64, 127)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want[sel])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(stream())
    for sel2, flip in ([[4, 1, 7], False], [[6, 2, 2], True]):
        new_raw = (255 - raw) if flip else raw                                # new bytes in the same buffer
        new_hw = hw[sel2].clone()
        if flip:
            new_hw[1] = 0                                                     # and a frame that went missing
        rd.copy_(new_raw)
        od.copy_(offset[sel2])
        hd.copy_(new_hw)
        out.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        ref = ref_resize.resize_table(new_raw.numpy(), offset[sel2].numpy(), new_hw.numpy(), c, size, 64, 127)
        assert torch.equal(out.cpu(), torch.from_numpy(ref)), sel2


def test_host_rejections_launch_nothing(hip):
    from video_classification_amd import _lib
    lib = hip.lib
    c, size = 5, 8
    src = torch.zeros(2 * 9 * 7 * c, dtype=torch.uint8, device=DEV)
    offset, hw = torch.tensor([0, 315], device=DEV), torch.tensor([[9, 7], [9, 7]], dtype=torch.int32, device=DEV)
    out = torch.full((2, size, size, c), 9, dtype=torch.uint8, device=DEV)

    def good():
        d = _lib.new_resize_desc()
        d.src, d.src_bytes, d.offset, d.hw, d.out = src.data_ptr(), src.numel(), offset.data_ptr(), hw.data_ptr(), out.data_ptr()
        d.frames, d.c, d.size, d.max_side, d.fill, d.out_frame_stride = 2, c, size, 9, 127, size * size * c
        return d
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 68), ("struct_size", 80), ("src", None), ("offset", None),
                         ("hw", None), ("out", None), ("frames", 0), ("c", 0), ("c", -1), ("size", 0), ("max_side", 0),
                         ("max_side", -3), ("src_bytes", -1), ("out_frame_stride", size * size * c - 1), ("fill", -1), ("fill", 256)]:
        d = good()
        setattr(d, field, value)
        assert lib.sfk_u8_pad_resize_cubic(B(d), stream()) == -1, (field, value)
    for fields in [{"frames": (1 << 23) // 8 + 1}, {"max_side": 667, "c": 21, "size": 192, "out_frame_stride": 192 * 192 * 21},
                   {"max_side": 4000}]:
        d = good()
        for k, v in fields.items():
            setattr(d, k, v)
        assert lib.sfk_u8_pad_resize_cubic(B(d), stream()) == -2, fields
    torch.cuda.synchronize()
    assert bool((out == 9).all())
    assert lib.sfk_u8_pad_resize_cubic(B(good()), stream()) == 0              # the descriptor they were all derived from
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                             # zeros resized are zeros


def _ragged(t, seed, lo=5, hi=40):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (int(torch.randint(lo, hi + 1, (1,), generator=g)), int(torch.randint(lo, hi + 1, (1,), generator=g)), 21),
                          generator=g, dtype=torch.uint8) for _ in range(t)]


def test_frame_pool_add_raw_then_gather(hip):
    size, T = 16, 4
    a, b = FramePool(DEV, hip), FramePool(DEV, hip)
    got, want, sent = [], [], 0
    for v, f in enumerate((3, 11)):
        frames = _ragged(f, seed=v)
        win = uniform_windows(f, T)
        item = make_raw_pooled_item("k", win, 0, lambda i: None if (v, i) == (1, 2) else frames[i])
        kept = [fr for i, fr in enumerate(frames) if (v, i) != (1, 2) and i in set(win.flatten().tolist())]
        resized = torch.stack([torch.from_numpy(ref_resize.pad_resize_int(fr.numpy(), size)) for fr in kept])
        ba = a.add_raw(item["k_rawpool"], item["raw_hw"], size, item["windows"])
        bb = b.add(resized, item["windows"])
        assert ba == bb
        sent += item["k_rawpool"].numel()
        got.append(a.gather(a.rows(ba, item["windows"])))
        want.append(b.gather(b.rows(bb, item["windows"])))
    torch.cuda.synchronize()
    assert a.bytes_uploaded == sent and tuple(a.arena.shape[1:]) == (size, size, 21)
    assert torch.equal(torch.cat(got).cpu(), torch.cat(want).cpu())
    assert a.live == b.live == {0: 3, 3: 7} and torch.equal(a.arena[:10].cpu(), b.arena[:10].cpu())
    fill = torch.cat(want).cpu()[1 + 0, 2]                                    # video 1, window 0, frame 2: the missing one
    assert float(fill.min()) == float(fill.max())


def _cfg(tmp_path, u8_stem=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.R3D_INPUT = "CropLHand"                       # 64 x 64 crops
    cfg.MODEL.NAME = "slowfast-test"
    cfg.MODEL.U8_STEM = u8_stem
    cfg.DEBUG = True
    return cfg


def _resized_frames(raw, hw, size=64):
    out, at = [], 0
    for h, w in hw.tolist():
        if h == 0:
            out.append(torch.full((size, size, 21), MISSING_BYTE, dtype=torch.uint8))
            continue
        out.append(torch.from_numpy(ref_resize.pad_resize_int(raw[at:at + h * w * 21].reshape(h, w, 21).numpy(), size)))
        at += h * w * 21
    return torch.stack(out)


class _Pooled(torch.utils.data.Dataset):
    """raw pooled videos as the pooled items of their reference-resized frames"""

    def __init__(self, raw_set):
        self.s = raw_set

    def __len__(self):
        return len(self.s)

    def __getitem__(self, i):
        it = self.s[i]
        return {"CropLHand_pool": _resized_frames(it["CropLHand_rawpool"], it["raw_hw"]), "windows": it["windows"], "label": it["label"]}


def test_trainer_run_eval_on_raw_pooled_videos_equals_the_pooled_one(hip, tmp_path):
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = _cfg(tmp_path)
    tr_set = SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
    te_set = SyntheticChalearn(cfg, "test", num_videos=3, seed=2, raw=True, frames_per_video=(3, 14), raw_side=(20, 90))
    loader = torch.utils.data.DataLoader(tr_set, batch_size=2, shuffle=False, drop_last=True)
    raw = torch.utils.data.DataLoader(te_set, batch_size=2, shuffle=False, collate_fn=lambda x: x)
    pooled = torch.utils.data.DataLoader(_Pooled(te_set), batch_size=2, shuffle=False, collate_fn=lambda x: x)
    trainer = Trainer(cfg, train_loader=loader, test_loader=raw, device=DEV, backend=hip)
    logits = []
    fwd = trainer.model.forward
    trainer.model.forward = lambda x: (lambda y: (logits.append(y.float().cpu().clone()), y)[1])(fwd(x))
    a = trainer.run_eval(pooled)
    la, logits[:] = list(logits), []
    got = trainer.run_eval()
    assert len(la) == len(logits) > 0 and all(torch.equal(p, q) for p, q in zip(la, logits))
    assert got["sv"] == a["sv"] == te_set.nclips and np.array_equal(got["t"], a["t"]) and got["acc"] == a["acc"]
    assert np.array_equal(got["ps"], a["ps"])
    assert trainer.frame_pool.bytes_uploaded == sum(te_set[i]["CropLHand_rawpool"].numel() for i in range(len(te_set)))
    assert not trainer.frame_pool.live


@pytest.mark.parametrize("u8_stem", [False, True], ids=["float_clip", "u8_stem"])
def test_prepare_data_from_a_raw_batch_equals_the_u8_batch_of_resized_frames(hip, tmp_path, u8_stem):
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = _cfg(tmp_path, u8_stem)
    raw_set = SyntheticChalearn(cfg, "train", num_videos=2, seed=3, raw=True, raw_side=(20, 90))
    te_set = SyntheticChalearn(cfg, "test", num_videos=1, seed=2, as_uint8=True)
    trainer = Trainer(cfg, train_set=raw_set, test_set=te_set, device=DEV, backend=hip)        # the mini model
    assert trainer.train_loader.collate_fn is collate_raw
    items = [raw_set[0], raw_set[1]]
    rb = collate_raw(items)
    ub = {"CropLHand_u8": torch.stack([_resized_frames(it["CropLHand_raw"], it["raw_hw"]) for it in items]),
          "crop": rb["crop"].clone(), "label": rb["label"].clone()}
    xr, yr = trainer.mm.prepare_data(rb)
    xu, yu = trainer.mm.prepare_data(ub)
    torch.cuda.synchronize()
    assert torch.equal(yr.cpu(), yu.cpu())
    for p, q in zip(xr, xu):
        if u8_stem:
            assert torch.equal(p.frames.cpu(), q.frames.cpu()) and torch.equal(p.crop.cpu(), q.crop.cpu()) and (p.c0, p.c, p.pad) == (q.c0, q.c, q.pad)
        else:
            assert torch.equal(p.cpu(), q.cpu())
    trainer.model.eval()
    with torch.no_grad():
        lr = trainer.model(xr).float().cpu().clone()
        lu = trainer.model(xu).float().cpu().clone()
    assert torch.equal(lr, lu) and bool(torch.isfinite(lr).all())
