"""sfk_roi_resize_ragged (include/sfk_roi_ragged.h) on an MI355X: bit equality with sfk_roi_resize on each clip's cropped frames
stacked, bit equality with sfk_roi_resize_pool on the WHOLE frames with the untranslated boxes (a resize reads nothing outside
its box), 2e-6 against CPU F.interpolate, offsets and rectangles that must read as missing frames, guard bands and channel
sub-ranges, box and crop values far out of range, an arena beyond 2^31 bytes, reproducibility and a captured graph following
new tables, and ResidentGestureSet(store='box') / the v2 Trainer with MODEL.RESIDENT_STORE: box on the device."""
import math

import pytest
import torch

from emu_roi_ragged import materialise_ragged
from emu_v2 import clamp_box, roi_resize_ref
from test_gpu_roi_pool import F, FILL, H, I32_MAX, I32_MIN, ROWS, W, big_frames, run_pool, run_stacked, scaled_boxes, small_pool
from test_gpu_v2 import BOXES
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import ResidentGestureSet, RoiResize, byte_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
_cache = {}


def pack(frames, clips, lead=1, tail=0):
    """clips: [(frame indices, (x1, y1, x2, y2))].  Every clip's distinct frames, cropped to its rectangle, packed end to end
    in one byte arena -- each block pushed off the multiples of 4 by a byte where it would start on one -- then ``tail`` more
    bytes and the padding to a multiple of 4.  -> (arena uint8 on the device, offset (N, T) int64, hw (N, 2) int32)"""
    cpu = frames.cpu()
    chunks, at, offset, hw = [torch.zeros(lead, dtype=torch.uint8)], lead, [], []
    for rows, (x1, y1, x2, y2) in clips:
        if at % 4 == 0:
            chunks.append(torch.full((1,), 0xEE, dtype=torch.uint8))
            at += 1
        where = {}
        for f in rows:
            if f not in where:
                block = cpu[f, y1:y2, x1:x2].contiguous().view(-1)
                where[f] = at
                chunks.append(block)
                at += block.numel()
        offset.append([where[f] for f in rows])
        hw.append([y2 - y1, x2 - x1])
    chunks.append(torch.full((tail + (-(at + tail)) % 4,), 0xEE, dtype=torch.uint8))
    arena = torch.cat(chunks)
    assert arena.numel() % 4 == 0
    return arena.to(DEV), torch.tensor(offset, dtype=torch.int64), torch.tensor(hw, dtype=torch.int32)


def rect_for(box, kind, h, w):
    """a rectangle that contains the clamped box: the whole frame, the box itself, or one with an odd origin and odd sizes"""
    x1, y1, x2, y2 = clamp_box(box, h, w)
    if kind == 0:
        return 0, 0, w, h
    if kind == 1:
        return x1, y1, x2, y2
    rx1, ry1 = (x1 - 1) | 1 if x1 > 0 else 0, (y1 - 1) | 1 if y1 > 0 else 0
    rx2 = x2 if (x2 - rx1) % 2 == 1 or x2 == w else x2 + 1
    ry2 = y2 if (y2 - ry1) % 2 == 1 or y2 == h else y2 + 1
    return rx1, ry1, rx2, ry2


def small_case():
    """the twelve scaled boxes plus a 1-pixel-wide and a 1-pixel-tall one, each clip in its own rectangle of the small frames"""
    if "small" not in _cache:
        boxes = scaled_boxes().tolist() + [[40, 5, 41, 50], [7, 33, 70, 34]]
        rects = [rect_for(b, n % 3, H, W) for n, b in enumerate(boxes[:12])] + [(40, 5, 41, 50), (7, 33, 70, 34)]
        rows = [ROWS[n % len(ROWS)] for n in range(len(boxes))]
        arena, offset, hw = pack(small_pool(), list(zip(rows, rects)))
        assert all(int(o) % 4 for o in offset.view(-1)[::3])                  # no block starts on a dword
        assert any(r[0] % 2 and r[1] % 2 and (r[2] - r[0]) % 2 and (r[3] - r[1]) % 2 for r in rects)
        assert [45, 1] in hw[12:].tolist() and [1, 63] in hw[12:].tolist() and [H, W] in hw.tolist()
        assert any(tuple(r) == clamp_box(b, H, W) and tuple(r) != (0, 0, W, H) for r, b in zip(rects, boxes))
        origin = torch.tensor([[r[0], r[1], r[0], r[1]] for r in rects], dtype=torch.int32)
        box = torch.tensor(boxes, dtype=torch.int32)
        _cache["small"] = (arena, offset.to(DEV), hw.to(DEV), (box - origin).to(DEV), box.to(DEV),
                           torch.tensor(rows, dtype=torch.int32, device=DEV))
    return _cache["small"]


def run_ragged(arena, offset, hw, box, s, aa, dtype, crop=None, pad=0, fill=FILL, max_hw=(H, W), be=None, **kw):
    be = be or HipBackend()
    out = torch.full((offset.shape[0], offset.shape[1], 7, s, s), float("nan"), dtype=dtype, device=DEV)
    be.roi_resize_ragged(arena, offset, hw, byte_lut().to(DEV), fill, box, out, aa, crop, pad, max_hw=max_hw, **kw)(
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def stacked_clip_by_clip(arena, offset, hw, box, s, aa, dtype, crop, pad, fill, max_hw):
    """sfk_roi_resize on each clip's frames materialised from the arena (a missing frame as fill bytes), and those clips"""
    a, clips, outs = arena.cpu(), [], []
    for n in range(offset.shape[0]):
        clips.append(materialise_ragged(a, offset[n].cpu(), hw[n].cpu(), fill, max_hw))
        outs.append(run_stacked(clips[-1].to(DEV), box[n:n + 1], s, aa, dtype, None if crop is None else crop[n:n + 1], pad))
    return torch.cat(outs), clips


def check_all(arena, offset, hw, box, s, aa, crop, pad, fill=FILL, max_hw=(H, W)):
    """f32 and bf16: bit-equal to sfk_roi_resize clip by clip, f32 within 2e-6 of the CPU reference, bf16 the f32 rounded"""
    got = run_ragged(arena, offset, hw, box, s, aa, torch.float32, crop, pad, fill, max_hw)
    assert torch.isfinite(got).all()
    want, clips = stacked_clip_by_clip(arena, offset, hw, box, s, aa, torch.float32, crop, pad, fill, max_hw)
    assert torch.equal(got, want)
    ref = torch.cat([roi_resize_ref(c, byte_lut(), box[n:n + 1].cpu(), s, s, aa, None if crop is None else crop[n:n + 1].cpu(), pad)
                     for n, c in enumerate(clips)])
    err = float((got.cpu() - ref).abs().max())
    print("max abs error against the CPU reference", err)
    assert err <= 2e-6, err
    gb = run_ragged(arena, offset, hw, box, s, aa, torch.bfloat16, crop, pad, fill, max_hw)
    assert torch.equal(gb, stacked_clip_by_clip(arena, offset, hw, box, s, aa, torch.bfloat16, crop, pad, fill, max_hw)[0])
    assert torch.equal(gb, got.to(torch.bfloat16))          # round to nearest even of the f32 result
    return got


# ------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize("s", [32, 80])
@pytest.mark.parametrize("crop_mode", [None, "zero", "max"])
@pytest.mark.parametrize("aa", [False, True], ids=["linear", "antialias"])
def test_ragged_equals_roi_resize_on_the_cropped_frames_and_the_pool_on_the_whole_ones(aa, crop_mode, s):
    arena, offset, hw, box, whole_box, index = small_case()
    pad, n = s // 10, box.shape[0]
    crop = None if crop_mode is None else torch.full((n, 2), 0 if crop_mode == "zero" else 2 * pad, dtype=torch.int32, device=DEV)
    got = check_all(arena, offset, hw, box, s, aa, crop, pad)
    for dtype in (torch.float32, torch.bfloat16):           # the claim: cropping the source to a containing rectangle changes nothing
        want = run_pool(small_pool(), index, whole_box, s, aa, dtype, crop, pad)
        assert torch.equal(got.to(dtype) if dtype == torch.bfloat16 else got, want)
        assert torch.equal(run_ragged(arena, offset, hw, box, s, aa, dtype, crop, pad), want)


# ------------------------------------------------------------------ 2. missing frames at the v2 geometry
def big_case():
    """240 x 320 x 7 frames: clip 0 in a 150 x 200 rectangle, clip 1 in a 97 x 131 one, clip 2 whole, 3 frames each"""
    if "big" not in _cache:
        rects = [(60, 40, 260, 190), (101, 77, 232, 174), (0, 0, 320, 240)]
        arena, offset, hw = pack(big_frames(), list(zip([[0, 1, 2], [5, 3, 1], [4, 2, 0]], rects)), lead=3)
        assert arena.numel() - (int(offset[2, 0]) + 240 * 320 * 7 * 3) < 4 and hw.tolist() == [[150, 200], [97, 131], [240, 320]]
        origin = torch.tensor([[r[0], r[1], r[0], r[1]] for r in rects], dtype=torch.int32)
        box = torch.tensor([[70, 45, 250, 180], [110, 80, 230, 170], BOXES["down"][0]], dtype=torch.int32) - origin
        crop = torch.tensor([[38, 0], [7, 31], [19, 19]], dtype=torch.int32)
        _cache["big"] = (arena, offset, hw, box.to(DEV), crop.to(DEV))
    return _cache["big"]


def big_result():
    """clips 0 and 1 of big_case to 192, antialias, a crop: checked once, kept for the large-arena test"""
    if "big_result" not in _cache:
        arena, offset, hw, box, crop = big_case()
        _cache["big_result"] = check_all(arena, offset[:2].to(DEV), hw[:2].to(DEV), box[:2], 192, True, crop[:2], 19, max_hw=(240, 320))
    return _cache["big_result"]


def test_ragged_at_the_v2_geometry():
    big_result()
    arena, offset, hw, box, crop = big_case()                                 # the whole frame, the last block of the arena
    check_all(arena, offset[1:].to(DEV), hw[1:].to(DEV), box[1:], 192, True, crop[1:], 19, max_hw=(240, 320))


def test_offsets_and_rectangles_that_do_not_lie_in_the_arena_read_as_missing_frames():
    arena, offset, hw, box, crop = big_case()
    nbytes = arena.numel()
    off = offset[:2].clone()
    off[0, 1], off[0, 2] = -1, I64_MIN
    off[1] = torch.tensor([I64_MAX, nbytes - 1, nbytes - 97 * 131 * 7 + 1])   # the last: ends one byte past the arena
    flush = offset[:2].clone()
    flush[1, 2] = nbytes - 97 * 131 * 7                                       # ends exactly with the arena: a frame
    inside = torch.zeros(1, 1, 1, 192, 192, dtype=torch.bool, device=DEV)     # where the crop shift leaves the resized image
    inside[..., :192 - 19, 19:] = True                                        # clip 0: (top - pad, left - pad) = (19, -19)
    for fill in (FILL, 0, 255):
        got = check_all(arena, off.to(DEV), hw[:2].to(DEV), box[:2], 192, True, crop[:2], 19, fill, max_hw=(240, 320))
        const = float(byte_lut()[fill])
        for n, t in ((0, 1), (0, 2), (1, 0), (1, 1), (1, 2)):                 # the constant image, resized: the constant
            assert bool((((got[n, t] - const).abs() <= 2e-6) | (got[n, t] == 0)).all()), (fill, n, t)
        assert bool(((got[0, 1:] - const).abs() <= 2e-6)[inside.expand(1, 2, 7, 192, 192)[0]].all())
        assert not bool((got[0, 1:] != 0)[~inside.expand(1, 2, 7, 192, 192)[0]].any())
        assert float((got[0, 0] - const).abs().max()) > 0.1                   # (the one frame that is there is not constant)
    got = check_all(arena, flush.to(DEV), hw[:2].to(DEV), box[:2], 192, True, crop[:2], 19, max_hw=(240, 320))
    assert float((got[1, 2] - float(byte_lut()[FILL])).abs().max()) > 0.1
    # hw rows outside [1, max_hw]: every frame of that clip is missing, whatever its offsets say
    for row in ((0, 131), (97, 0), (-5, 131), (97, -1), (241, 131), (97, 321), (I32_MIN, I32_MAX), (I32_MAX, I32_MAX)):
        bad = hw[:2].clone()
        bad[1] = torch.tensor(row, dtype=torch.int32)
        got = check_all(arena, offset[:2].to(DEV), bad.to(DEV), box[:2], 192, True, None, 0, max_hw=(240, 320))
        assert float((got[1] - float(byte_lut()[FILL])).abs().max()) <= 2e-6, row
        assert torch.equal(got[0], run_ragged(arena, offset[:1].to(DEV), hw[:1].to(DEV), box[:1], 192, True, torch.float32,
                                              max_hw=(240, 320))[0])
    # a rectangle above max_hw although it lies in the arena
    got = check_all(arena, offset[:2].to(DEV), hw[:2].to(DEV), box[:2], 192, True, None, 0, max_hw=(149, 200))
    assert float((got[0] - float(byte_lut()[FILL])).abs().max()) <= 2e-6 < float((got[1] - float(byte_lut()[FILL])).abs().max())


# ------------------------------------------------------------------ 3. guard bands and channel ranges
def test_guard_bands_and_channel_ranges():
    arena, offset, hw, box, _, _ = small_case()
    be, s, lut = HipBackend(), 32, byte_lut().to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    sel = [0, 4, 8, 13]
    offset, hw, box = offset[sel].clone(), hw[sel].contiguous(), box[sel].contiguous()
    offset[0, 0], offset[2, 1], offset[2, 2] = -1, -1, arena.numel()
    full = run_ragged(arena, offset, hw, box, s, True, torch.float32)
    for dtype in (torch.float32, torch.bfloat16):
        guard, numel = 1024, 4 * 3 * 9 * s * s
        flat = torch.full((guard + numel + guard,), float("nan"), dtype=dtype, device=DEV)
        out = flat[guard:guard + numel].view(4, 3, 9, s, s)
        be.roi_resize_ragged(arena, offset, hw, lut, FILL, box, out, True, c_off=1, max_hw=(H, W))(st)
        torch.cuda.synchronize()
        assert torch.isnan(flat[:guard]).all() and torch.isnan(flat[-guard:]).all()
        assert torch.isnan(out[:, :, 0]).all() and torch.isnan(out[:, :, 8]).all()
        assert torch.equal(out[:, :, 1:8], full.to(dtype))
        out.fill_(float("nan"))
        be.roi_resize_ragged(arena, offset, hw, lut, FILL, box, out, True, c0=2, c=3, c_off=4, max_hw=(H, W))(st)   # channels 2..4 -> planes 4..6
        torch.cuda.synchronize()
        assert torch.equal(out[:, :, 4:7], full[:, :, 2:5].to(dtype))
        assert torch.isnan(out[:, :, :4]).all() and torch.isnan(out[:, :, 7:]).all()
        assert torch.isnan(flat[:guard]).all() and torch.isnan(flat[-guard:]).all()


# ------------------------------------------------------------------ 4. far-out tables
def test_box_and_crop_values_far_out_of_range_stay_finite():
    arena, offset, hw, _, _, _ = small_case()
    sel = [0, 1, 2, 5, 12, 13]                              # whole, exact, odd, odd, 1 wide, 1 tall
    offset, hw = offset[sel].contiguous(), hw[sel].contiguous()
    box = torch.tensor([[-50, 300, -3, 250], [400, -9, 1000, 2], [I32_MIN, I32_MIN, I32_MAX, I32_MAX],
                        [I32_MAX, I32_MAX, I32_MIN, I32_MIN], [W, H, W, H], [-1, -1, 0, 0]], dtype=torch.int32, device=DEV)
    crop = torch.tensor([[-2 ** 30, 2 ** 30], [10 ** 6, -10 ** 6], [0, 10 ** 6], [-7, 3], [2 ** 30, 2 ** 30], [5, -10 ** 6]],
                        dtype=torch.int32, device=DEV)
    for s in (32, 80):
        for aa in (False, True):
            for cr in (None, crop):
                got = run_ragged(arena, offset, hw, box, s, aa, torch.float32, cr, 3)
                assert torch.isfinite(got).all()
                assert torch.equal(got, stacked_clip_by_clip(arena, offset, hw, box, s, aa, torch.float32, cr, 3, FILL, (H, W))[0])
    assert not run_ragged(arena, offset, hw, box, 32, True, torch.float32, crop, 3)[[0, 1, 2, 4, 5]].any()   # shifted wholly outside


# ------------------------------------------------------------------ 5. an arena beyond 2^31 bytes
def test_an_arena_beyond_2_to_the_31_bytes():
    """2^31 + 2^24 bytes, uninitialised but for the two clips' blocks copied above 2^31: a 32-bit byte offset would read
    elsewhere, or nothing"""
    want = big_result()
    small, offset, hw, box, crop = big_case()
    used = int(offset[2, 0])                                                  # clips 0 and 1 lie below this
    nbytes = 2 ** 31 + 2 ** 24
    try:
        arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    except RuntimeError as e:                                                 # (torch's OutOfMemoryError is one)
        pytest.skip(f"no room for a {nbytes} byte arena on this device: {e}")
    shift = 2 ** 31 + 4                                                       # keeps every block's byte phase
    assert shift + used <= nbytes
    arena[shift:shift + used].copy_(small[:used])
    far = (offset[:2] + shift).to(DEV)
    assert int(far.min()) > 2 ** 31
    got = run_ragged(arena, far, hw[:2].to(DEV), box[:2], 192, True, torch.float32, crop[:2], 19, max_hw=(240, 320))
    assert torch.equal(got, want)
    gb = run_ragged(arena, far, hw[:2].to(DEV), box[:2], 192, True, torch.bfloat16, crop[:2], 19, max_hw=(240, 320))
    assert torch.equal(gb, want.to(torch.bfloat16))
    del arena
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. determinism and graphs
def test_two_runs_are_bit_equal_and_a_graph_follows_new_tables():
    arena, all_offset, all_hw, all_box, _, _ = small_case()
    be, s, lut = HipBackend(), 80, byte_lut().to(DEV)
    offset, hw, box = all_offset[:4].clone(), all_hw[:4].clone(), all_box[:4].clone()
    crop = torch.tensor([[0, 16], [8, 8], [16, 0], [3, 11]], dtype=torch.int32, device=DEV)
    a = run_ragged(arena, offset, hw, box, s, True, torch.float32, crop, 8, be=be)
    b = run_ragged(arena, offset, hw, box, s, True, torch.float32, crop, 8, be=be)
    assert torch.equal(a, b)
    out = torch.empty(4, 3, 7, s, s, device=DEV)
    run = be.roi_resize_ragged(arena, offset, hw, lut, FILL, box, out, True, crop, 8, max_hw=(H, W))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    tables = [([4, 5, 12, 7], torch.tensor([[16, 16], [0, 0], [5, 9], [12, 1]], dtype=torch.int32), {(1, 0): -1}),
              ([8, 13, 10, 11], torch.tensor([[1, 2], [16, 0], [0, 16], [8, 8]], dtype=torch.int32), {(2, 0): arena.numel(), (2, 2): -1})]
    for k, (sel, cr, missing) in enumerate(tables):
        off = all_offset[sel].clone()
        for (n, t), v in missing.items():
            off[n, t] = v
        offset.copy_(off), hw.copy_(all_hw[sel]), box.copy_(all_box[sel]), crop.copy_(cr)
        g.replay()
        torch.cuda.synchronize()
        want, clips = stacked_clip_by_clip(arena, offset, hw, box, s, True, torch.float32, crop, 8, FILL, (H, W))
        assert torch.equal(out, want), k
        ref = torch.cat([roi_resize_ref(c, byte_lut(), box[n:n + 1].cpu(), s, s, True, crop[n:n + 1].cpu(), 8) for n, c in enumerate(clips)])
        assert float((out.cpu() - ref).abs().max()) <= 2e-6, k


# ------------------------------------------------------------------ 7. ResidentGestureSet(store='box') and the v2 Trainer on the device
def _cfg(dtype="fp32", root="/nonexistent", jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "gesture-v2"
    cfg.MODEL.INPUT_SIZE = 64
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.DTYPE = dtype
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


@pytest.mark.parametrize("dtype,augment", [("fp32", False), ("bf16", True)])
def test_box_store_on_the_device_equals_its_replayed_plan_on_the_whole_frames(dtype, augment):
    from video_classification_amd import gesture_v2 as v2
    cfg = _cfg(dtype)
    ds = v2.SyntheticGesture(cfg, "train", num_videos=5, seed=3, h=H, w=W, min_box=8, videos=True, frames_per_video=(2, 9))
    cost = []
    for v in range(5):
        b = ds.frame_boxes(v)
        x1, y1, x2, y2 = max(0, int(b[:, 0].min())), max(0, int(b[:, 1].min())), min(W, int(b[:, 2].max())), min(H, int(b[:, 3].max()))
        cost.append(ds.seq_len(v) * (y2 - y1) * (x2 - x1) * 7)
    nbytes = 2 * (4 * H * W * 7 + 16) + sum(cost) // 2                        # half resident, half spilled
    r = ResidentGestureSet(ds, cfg, DEV, batch_size=2, drop_last=False, seed=4, augment=augment, store="box", capacity_bytes=nbytes)
    roi = RoiResize(64, DEV, out_dtype=r.out_dtype)
    uploaded = []
    for e in range(3):
        plan = r.plan(e)
        got = list(r.epoch(e))
        torch.cuda.synchronize()
        assert len(got) == len(plan) == 3
        for batch, (videos, indices, box, crop, _) in zip(got, plan):
            assert (crop is not None) == augment and batch["clip_v2"].dtype == r.out_dtype and batch["clip_v2"].is_cuda
            frames = torch.stack([ds.video_item(v, indices[n].tolist())["frames_pool"] for n, v in enumerate(videos)])
            assert torch.equal(batch["clip_v2"], roi(frames, box, crop))
            assert batch["label"].tolist() == [ds.label(v) for v in videos]
        uploaded.append(r.bytes_uploaded)
    assert 0 < r.resident_videos < 5 and r.spilled_clips == 5 - r.resident_videos and 0 < r.spill_peak <= 8
    assert r.resident_bytes_used == sum(cost[v] for v, ok in r._resident.items() if ok)
    assert uploaded[2] - uploaded[1] == sum(
        len(set(row.tolist())) * int(bx[3] - bx[1]) * int(bx[2] - bx[0]) * 7
        for entry in r.plan(2) for v, row, bx in zip(entry[0], entry[1], entry[2]) if not r._resident[v])


def test_v2_trainer_trains_the_same_from_the_box_store_and_uploads_nothing_in_the_second_epoch(tmp_path):
    """MODEL.RESIDENT_STORE: box against frame, same seed: the clips of every step are EQUAL, and after the first step so are
    the loss and every parameter the step computes reproducibly.  That is all of them but the two stems' filters, once the
    engine runs with deterministic_wgrad: the stem filter-gradient kernels flush with atomic adds under every switch
    (tests/test_gpu_model.py), so two runs of the SAME store already differ there (measured on the 'frame' store: about 1e-4
    of the parameters, by at most 1.5e-8 after six steps).  The stems' filters are held to 4 ulp of the largest of them per
    step: each run rounds its update into the fp32 master once (half an ulp each) and the reordered sums move lr * dW by
    about as much again -- a wrong clip would move them by lr * |dW|, orders of magnitude more.  The comparison is made after
    ONE step (an epoch of one batch): later steps read the stems through their bf16 shadow, where a last-bit difference of
    the master can flip a rounding and then reach everything."""
    from video_classification_amd import gesture_v2 as v2
    out = {}
    for store in ("frame", "box"):
        torch.manual_seed(0)
        cfg = _cfg("bf16", root=tmp_path, jitter=True)
        cfg.CHALEARN.BATCH_SIZE = 4
        cfg.MODEL.LR = 1e-3
        cfg.MODEL.RESIDENT_TRAIN = True
        cfg.MODEL.RESIDENT_STORE = store
        cfg.MODEL.RESIDENT_GB = 100 * H * W * 7 / 2 ** 30
        tr = v2.SyntheticGesture(cfg, "train", num_videos=4, seed=1, h=H, w=W, min_box=8, videos=True, frames_per_video=(3, 9))
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
        t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
        assert isinstance(t.resident, ResidentGestureSet) and t.resident.store == store
        eng = t.model.engine
        assert not eng._plans                                                 # built at the first step: the switch below is read then
        eng.deterministic_wgrad = True
        seen, prepare = [], t.mm.prepare_data
        t.mm.prepare_data = lambda batch: (seen.append({k: v.clone() for k, v in batch.items()}), prepare(batch))[1]
        t.train_loader = None                                                 # the loader path is not taken
        loss, _ = t.train_epoch()
        torch.cuda.synchronize()
        assert math.isfinite(loss) and t.step.steps == 1 and int(eng.sgd_step[0]) == 1
        params = eng.P.data.clone()
        uploaded = t.resident.bytes_uploaded
        assert t.resident.resident_videos == 4 and uploaded > 0
        t.epoch = 1
        second, _ = t.train_epoch()
        torch.cuda.synchronize()
        assert math.isfinite(second) and t.resident.bytes_uploaded == uploaded and t.resident.spilled_clips == 0
        stems = torch.zeros(params.numel(), dtype=torch.bool, device=DEV)
        for L in eng.layers:
            if L.cb.is_stem:
                stems[L.w_off:L.w_off + L.w_numel] = True
        out[store] = (loss, params, uploaded, seen, stems)
    (la, pa, ua, sa, stems), (lb, pb, ub, sb, _) = out["frame"], out["box"]
    assert len(sa) == len(sb) == 2
    for x, y in zip(sa, sb):                                                  # (cloned BEFORE the jitter ran in place)
        assert sorted(x) == sorted(y) == ["clip_v2", "jitter", "label"] and all(torch.equal(x[k], y[k]) for k in x)
    assert la == lb
    assert 0 < int(stems.sum()) < stems.numel() and torch.equal(pa[~stems], pb[~stems])
    top = float(pa[stems].abs().max())
    ulp = 2.0 ** (math.floor(math.log2(top)) - 23)
    err = float((pa[stems] - pb[stems]).abs().max())
    print("stem filters: largest", top, "ulp", ulp, "max abs difference between the stores", err)
    assert err <= 4 * ulp, (err, ulp)
    assert ub < ua == sum(tr.vframes) * H * W * 7
