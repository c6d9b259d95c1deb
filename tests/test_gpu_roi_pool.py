"""sfk_roi_resize_pool (include/sfk_roi_pool.h) on an MI355X: bit equality with sfk_roi_resize on the clips materialised from
the pool and 2e-6 against CPU F.interpolate (both antialias settings, every crop mode, f32 and bf16, boxes of every kind of
tests/test_gpu_v2.py), missing frames, guard bands and channel sub-ranges, box and crop values far out of range, a pool beyond
2^31 bytes, reproducibility and a captured graph following new tables, and ResidentGestureSet / the v2 Trainer on the device."""
import math

import pytest
import torch

from emu_roi_pool import materialise
from emu_v2 import roi_resize_ref
from test_gpu_v2 import BOXES
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import ResidentGestureSet, RoiResize, byte_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, F = 59, 83, 12              # odd height and width: every frame and row starts at another byte phase
FILL = 127
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
# frames shared by two clips with different boxes, descending order, repeats
ROWS = [[0, 1, 2], [2, 1, 0], [5, 5, 5], [11, 7, 0]]
_cache = {}


def small_pool():
    if "small" not in _cache:
        g = torch.Generator().manual_seed(11)
        _cache["small"] = torch.randint(0, 256, (F, H, W, 7), generator=g, dtype=torch.uint8).to(DEV)
    return _cache["small"]


def big_frames():
    """(6, 240, 320, 7) uint8 on the device"""
    if "big" not in _cache:
        g = torch.Generator().manual_seed(12)
        _cache["big"] = torch.randint(0, 256, (6, 240, 320, 7), generator=g, dtype=torch.uint8).to(DEV)
    return _cache["big"]


def scaled_boxes():
    """the twelve boxes of test_gpu_v2.BOXES, scaled from 320 x 240 to the small frame: (12, 4) int32"""
    rows = [[x1 * W // 320, y1 * H // 240, x2 * W // 320, y2 * H // 240] for kind in BOXES.values() for x1, y1, x2, y2 in kind]
    return torch.tensor(rows, dtype=torch.int32)


def index_table(n):
    return torch.tensor([ROWS[i % len(ROWS)] for i in range(n)], dtype=torch.int32)


def run_pool(pool, index, box, s, aa, dtype, crop=None, pad=0, fill=FILL, be=None):
    be = be or HipBackend()
    out = torch.full((index.shape[0], index.shape[1], pool.shape[3], s, s), float("nan"), dtype=dtype, device=DEV)
    be.roi_resize_pool(pool, index, byte_lut().to(DEV), fill, box, out, aa, crop, pad)(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def run_stacked(clips, box, s, aa, dtype, crop=None, pad=0, be=None):
    be = be or HipBackend()
    out = torch.full((clips.shape[0], clips.shape[1], clips.shape[4], s, s), float("nan"), dtype=dtype, device=DEV)
    be.roi_resize(clips, byte_lut().to(DEV), box, out, aa, crop, pad)(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def check_all(pool, index, box, s, aa, crop, pad, fill=FILL):
    """f32 and bf16: bit-equal to sfk_roi_resize on the materialised clips, f32 within 2e-6 of the CPU reference"""
    clips = materialise(pool, index, fill).contiguous()
    got = run_pool(pool, index, box, s, aa, torch.float32, crop, pad, fill)
    assert torch.isfinite(got).all()
    assert torch.equal(got, run_stacked(clips, box, s, aa, torch.float32, crop, pad))
    want = roi_resize_ref(clips.cpu(), byte_lut(), box.cpu(), s, s, aa, None if crop is None else crop.cpu(), pad)
    err = float((got.cpu() - want).abs().max())
    print("max abs error against the CPU reference", err)
    assert err <= 2e-6, err
    gb = run_pool(pool, index, box, s, aa, torch.bfloat16, crop, pad, fill)
    assert torch.equal(gb, run_stacked(clips, box, s, aa, torch.bfloat16, crop, pad))
    assert torch.equal(gb, got.to(torch.bfloat16))          # round to nearest even of the f32 result
    return got


@pytest.mark.parametrize("s", [32, 80])                     # 32: reduces about 2.6x; 80: upsamples, two column tiles, one partial
@pytest.mark.parametrize("crop_mode", [None, "zero", "max"])
@pytest.mark.parametrize("aa", [False, True], ids=["linear", "antialias"])
def test_roi_resize_pool_equals_roi_resize_on_the_materialised_clips(aa, crop_mode, s):
    box = scaled_boxes().to(DEV)
    index = index_table(box.shape[0]).to(DEV)
    pad = s // 10
    crop = None if crop_mode is None else torch.full((box.shape[0], 2), 0 if crop_mode == "zero" else 2 * pad, dtype=torch.int32,
                                                     device=DEV)
    check_all(small_pool(), index, box, s, aa, crop, pad)


def big_result():
    """the 240 x 320 x 7 -> 192 case, 2 clips of 3 of 6 frames, antialias, a crop: checked once, kept for the large-pool test"""
    if "big_result" not in _cache:
        index = torch.tensor([[0, 1, 2], [5, 3, 1]], dtype=torch.int32, device=DEV)
        box = torch.tensor(BOXES["down"], dtype=torch.int32, device=DEV)
        crop = torch.tensor([[38, 0], [7, 31]], dtype=torch.int32, device=DEV)
        _cache["big_result"] = (index, box, crop, check_all(big_frames(), index, box, 192, True, crop, 19))
    return _cache["big_result"]


def test_roi_resize_pool_at_the_v2_geometry():
    big_result()


def test_missing_frames_guard_bands_and_channel_ranges():
    pool, be, s = small_pool(), HipBackend(), 32
    lut = byte_lut().to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    index = torch.tensor([[-1, 3, F], [I32_MAX, I32_MIN, 4], [2, -1, -1], [7, 8, 9]], dtype=torch.int32, device=DEV)
    box = scaled_boxes()[[0, 4, 8, 3]].to(DEV)
    for fill in (FILL, 0, 255):
        got = check_all(pool, index, box, s, True, None, 0, fill)
        assert float((got[0, 0] - byte_lut()[fill]).abs().max()) <= 2e-6      # the constant image, resized: the constant
    full = run_pool(pool, index, box, s, True, torch.float32)
    for dtype in (torch.float32, torch.bfloat16):
        guard, numel = 1024, 4 * 3 * 9 * s * s
        flat = torch.full((guard + numel + guard,), float("nan"), dtype=dtype, device=DEV)
        out = flat[guard:guard + numel].view(4, 3, 9, s, s)
        be.roi_resize_pool(pool, index, lut, FILL, box, out, True, c_off=1)(st)
        torch.cuda.synchronize()
        assert torch.isnan(flat[:guard]).all() and torch.isnan(flat[-guard:]).all()
        assert torch.isnan(out[:, :, 0]).all() and torch.isnan(out[:, :, 8]).all()
        assert torch.equal(out[:, :, 1:8], full.to(dtype))
        out.fill_(float("nan"))
        be.roi_resize_pool(pool, index, lut, FILL, box, out, True, c0=2, c=3, c_off=4)(st)     # channels 2..4 -> planes 4..6
        torch.cuda.synchronize()
        assert torch.equal(out[:, :, 4:7], full[:, :, 2:5].to(dtype))
        assert torch.isnan(out[:, :, :4]).all() and torch.isnan(out[:, :, 7:]).all()
        assert torch.isnan(flat[:guard]).all() and torch.isnan(flat[-guard:]).all()


def test_box_and_crop_values_far_out_of_range_stay_finite():
    pool = small_pool()
    index = index_table(6).to(DEV)
    box = torch.tensor([[-50, 300, -3, 250], [400, -9, 1000, 2], [I32_MIN, I32_MIN, I32_MAX, I32_MAX],
                        [I32_MAX, I32_MAX, I32_MIN, I32_MIN], [W, H, W, H], [-1, -1, 0, 0]], dtype=torch.int32, device=DEV)
    crop = torch.tensor([[-2 ** 30, 2 ** 30], [10 ** 6, -10 ** 6], [0, 10 ** 6], [-7, 3], [2 ** 30, 2 ** 30], [5, -10 ** 6]],
                        dtype=torch.int32, device=DEV)
    clips = materialise(pool, index, FILL).contiguous()
    for s in (32, 80):
        for aa in (False, True):
            for cr in (None, crop):
                got = run_pool(pool, index, box, s, aa, torch.float32, cr, 3)
                assert torch.isfinite(got).all()
                assert torch.equal(got, run_stacked(clips, box, s, aa, torch.float32, cr, 3))
    assert not run_pool(pool, index, box, 32, True, torch.float32, crop, 3)[[0, 1, 2, 4, 5]].any()   # shifted wholly outside


def test_a_pool_beyond_2_to_the_31_bytes():
    """4100 slots of 240 x 320 x 7 (2.2e9 bytes), uninitialised but for the last six: a 32-bit byte offset would read
    elsewhere"""
    index, box, crop, want = big_result()
    slots = 4100
    try:
        pool = torch.empty((slots, 240, 320, 7), dtype=torch.uint8, device=DEV)
    except RuntimeError as e:                                                 # (torch's OutOfMemoryError is one)
        pytest.skip(f"no room for a {slots * 240 * 320 * 7} byte pool on this device: {e}")
    assert (slots - 6) * pool.stride(0) > 2 ** 31
    pool[slots - 6:].copy_(big_frames())
    far = (index + (slots - 6)).contiguous()
    got = run_pool(pool, far, box, 192, True, torch.float32, crop, 19)
    assert torch.equal(got, want)
    gb = run_pool(pool, far, box, 192, True, torch.bfloat16, crop, 19)
    assert torch.equal(gb, want.to(torch.bfloat16))
    del pool
    torch.cuda.empty_cache()


def test_two_runs_are_bit_equal_and_a_graph_follows_new_tables():
    pool, be, s = small_pool(), HipBackend(), 80
    lut = byte_lut().to(DEV)
    boxes = scaled_boxes()
    index, box = index_table(4).to(DEV), boxes[:4].to(DEV)
    crop = torch.tensor([[0, 16], [8, 8], [16, 0], [3, 11]], dtype=torch.int32, device=DEV)
    a = run_pool(pool, index, box, s, True, torch.float32, crop, 8, be=be)
    b = run_pool(pool, index, box, s, True, torch.float32, crop, 8, be=be)
    assert torch.equal(a, b)
    out = torch.empty(4, 3, 7, s, s, device=DEV)
    run = be.roi_resize_pool(pool, index, lut, FILL, box, out, True, crop, 8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    tables = [(torch.tensor([[3, 2, 1], [-1, 0, 11], [6, 6, 7], [9, 10, 9]], dtype=torch.int32), boxes[4:8],
               torch.tensor([[16, 16], [0, 0], [5, 9], [12, 1]], dtype=torch.int32)),
              (torch.tensor([[11, 11, 11], [0, 1, 2], [F, 4, -1], [8, 2, 5]], dtype=torch.int32), boxes[8:12],
               torch.tensor([[1, 2], [16, 0], [0, 16], [8, 8]], dtype=torch.int32))]
    for k, (idx, bx, cr) in enumerate(tables):
        index.copy_(idx), box.copy_(bx), crop.copy_(cr)
        g.replay()
        torch.cuda.synchronize()
        clips = materialise(pool, index, FILL).contiguous()
        assert torch.equal(out, run_stacked(clips, box, s, True, torch.float32, crop, 8, be=be)), k
        want = roi_resize_ref(clips.cpu(), byte_lut(), box.cpu(), s, s, True, crop.cpu(), 8)
        assert float((out.cpu() - want).abs().max()) <= 2e-6, k


# ------------------------------------------------------------------ ResidentGestureSet and the v2 Trainer on the device
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
def test_resident_gesture_set_on_the_device_equals_its_replayed_plan(dtype, augment):
    from video_classification_amd import gesture_v2 as v2
    cfg = _cfg(dtype)
    ds = v2.SyntheticGesture(cfg, "train", num_videos=5, seed=3, h=H, w=W, min_box=8, videos=True, frames_per_video=(2, 9))
    cap = sum(ds.vframes) // 2 + 2 * 4                                       # half resident, half spilled
    r = ResidentGestureSet(ds, cfg, DEV, batch_size=2, drop_last=False, seed=4, capacity_frames=cap, augment=augment)
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
    assert uploaded[2] - uploaded[1] == sum(len(set(row.tolist())) for entry in r.plan(2) for v, row in zip(entry[0], entry[1])
                                            if not r._resident[v]) * H * W * 7


def test_v2_trainer_trains_from_the_resident_set_and_uploads_nothing_in_the_second_epoch(tmp_path):
    from video_classification_amd import gesture_v2 as v2
    cfg = _cfg("bf16", root=tmp_path, jitter=True)
    cfg.MODEL.LR = 1e-3
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 100 * H * W * 7 / 2 ** 30
    tr = v2.SyntheticGesture(cfg, "train", num_videos=5, seed=1, h=H, w=W, min_box=8, videos=True, frames_per_video=(3, 9))
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=H, w=W, min_box=8)
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    assert isinstance(t.resident, ResidentGestureSet) and t.resident.capacity == 100
    t.train_loader = None                                                     # the loader path is not taken
    loss, _ = t.train_epoch()
    assert math.isfinite(loss) and t.step.steps == 3 and int(t.model.engine.sgd_step[0]) == 3
    uploaded = t.resident.bytes_uploaded
    assert uploaded == sum(tr.vframes) * H * W * 7 and t.resident.resident_videos == 5
    t.epoch = 1
    loss, _ = t.train_epoch()
    assert math.isfinite(loss) and t.resident.bytes_uploaded == uploaded and t.resident.spilled_clips == 0
