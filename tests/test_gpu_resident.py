"""sfk_u8_pool_gather_crop on an MI355X (include/sfk_resident.h): bit-exactness against sfk_u8_normalize_crop (DevicePreprocess)
on the materialised clips with the same crop, in f32 and bf16, for never-aligned rows with scalar stores, aligned rows with
16-byte stores and a pad of 4, at the corners and the centre of the crop range and mixed per clip; an explicit pad; no crop
against sfk_u8_pool_gather; a pixel pitch wider than the channels read; missing frames and untouched memory around the output;
crop values far outside their range; reproducibility; a captured graph following new indices and crops; ResidentTrainSet
against its replayed plan; and one Trainer.train_epoch with MODEL.RESIDENT_TRAIN.  Both sides are table lookups of the same
bytes through the same table, so every comparison is torch.equal."""
import math

import pytest
import torch

from emu_resident import pool_gather_crop
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import (DevicePreprocess, PadResize, ResidentTrainSet, normalize_lut, raw_offsets,
                                                     unpool_item)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
KEY = "CropLHand"
FRAME = 64 * 64 * 21


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def stream():
    return torch.cuda.current_stream().cuda_stream


def frames_of(f, s, p, seed):
    return torch.randint(0, 256, (f, s, s, p), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def materialise(pool, idx, fill=127):
    """(N, T, S, S, P) uint8 clips of the index table, a missing frame as bytes of `fill`"""
    ext = torch.cat([pool, torch.full_like(pool[:1], fill)])
    i = idx.long()
    i = torch.where((i < 0) | (i >= pool.shape[0]), torch.tensor(pool.shape[0]), i)
    return ext[i]


def gather_crop(hip, pool_dev, idx, crop, pad, out_dtype, fill=127, c0=0, c=None):
    f, h, w, p = pool_dev.shape
    c = p - c0 if c is None else c
    out = torch.empty(idx.shape[0], idx.shape[1], c, h, w, dtype=out_dtype, device=DEV)
    crop = None if crop is None else crop.to(torch.int32).to(DEV)
    hip.u8_pool_gather_crop(pool_dev, idx.to(DEV), normalize_lut().to(DEV), fill, crop, pad, out, c0, c)(stream())
    torch.cuda.synchronize()
    return out.cpu()


SHAPES = {
    # name -> (F, S, P, index rows)
    "rows_of_65_bytes_scalar_stores": (5, 13, 5, [[0, 1, 2], [2, 3, 4], [4, 4, 0]]),
    "aligned_rows_vector_stores": (6, 16, 21, [[5, 5, 5, 5], [3, 0, 4, 1], [0, 5, 0, 5]]),
    "pad_of_4": (11, 40, 21, [[0, 1, 2, 3], [4, 5, 6, 7], [9, 10, 0, 1]]),
}


def crops_of(pad, n=3):
    """the four corners of [0, 2*pad]^2, the centre, and one that differs per clip"""
    m = 2 * pad
    same = [(0, 0), (0, m), (m, 0), (m, m), (pad, pad)]
    mixed = [(0, m), (m, pad), (pad - 1 if pad > 1 else 1, 0)]
    return [torch.tensor([c] * n, dtype=torch.int32) for c in same] + [torch.tensor(mixed[:n], dtype=torch.int32)]


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_crop_gather_is_bit_identical_to_normalize_crop_of_the_materialised_clips(hip, name, out_dtype):
    f, s, p, rows = SHAPES[name]
    pool = frames_of(f, s, p, seed=len(name))
    idx = torch.tensor(rows, dtype=torch.int32)
    clips, pd, pre = materialise(pool, idx), pool.to(DEV), DevicePreprocess(DEV, hip, out_dtype)
    pad = s // 10
    assert pad == {13: 1, 16: 1, 40: 4}[s]
    for crop in crops_of(pad):
        want = pre(clips, crop).cpu()
        got = gather_crop(hip, pd, idx, crop, pad, out_dtype)
        assert got.dtype == out_dtype and tuple(got.shape) == (3, idx.shape[1], p, s, s)
        assert torch.equal(got, want), crop.tolist()
        assert torch.equal(got, pool_gather_crop(pool, idx, normalize_lut(), 127, crop, pad, 0, p).to(out_dtype)), crop.tolist()


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_an_explicit_pad_of_5_at_13_pixels(hip, out_dtype):
    f, s, p, rows = SHAPES["rows_of_65_bytes_scalar_stores"]
    pool, idx = frames_of(f, s, p, seed=2), torch.tensor(rows, dtype=torch.int32)
    pre = DevicePreprocess(DEV, hip, out_dtype)
    for crop in crops_of(5):
        want = pre(materialise(pool, idx), crop, padding=5).cpu()
        assert torch.equal(gather_crop(hip, pool.to(DEV), idx, crop, 5, out_dtype), want), crop.tolist()


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_without_a_crop_it_is_the_pool_gather(hip, name, out_dtype):
    f, s, p, rows = SHAPES[name]
    pool, idx = frames_of(f, s, p, seed=7).to(DEV), torch.tensor(rows, dtype=torch.int32)
    idx[0, 0], idx[1, 1] = -1, f
    want = torch.empty(idx.shape[0], idx.shape[1], p, s, s, dtype=out_dtype, device=DEV)
    hip.u8_pool_gather(pool, idx.to(DEV), normalize_lut().to(DEV), 127, want)(stream())
    assert torch.equal(gather_crop(hip, pool, idx, None, 3, out_dtype), want.cpu())


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_pixel_pitch_wider_than_the_channels_read(hip, out_dtype):
    pool = frames_of(5, 13, 8, seed=3)                                        # pitch 8, channels 1..5 read
    idx = torch.tensor([[4, 0, 2], [1, 1, 3]], dtype=torch.int32)
    crop = torch.tensor([[2, 0], [1, 2]], dtype=torch.int32)
    want = DevicePreprocess(DEV, hip, out_dtype)(materialise(pool, idx)[..., 1:6].contiguous(), crop).cpu()
    assert torch.equal(gather_crop(hip, pool.to(DEV), idx, crop, 1, out_dtype, c0=1, c=5), want)
    # the same bytes as a strided view of a wider buffer: the strides come from the tensor
    wide = torch.zeros(5, 13, 16, 8, dtype=torch.uint8)
    wide[:, :, :13] = pool
    assert torch.equal(gather_crop(hip, wide.to(DEV)[:, :, :13], idx, crop, 1, out_dtype, c0=1, c=5), want)


def guarded(n_elems, shape, out_dtype, guard=64):
    buf = torch.full((n_elems + 2 * guard,), -7.0, dtype=out_dtype, device=DEV)
    out = buf[guard:guard + n_elems].view(shape)
    assert out.data_ptr() % 16 == 0
    return buf, out, guard


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("s", [13, 16])
def test_missing_frames_are_filled_then_padded_and_the_guards_stay(hip, s, out_dtype):
    f, p = 4, 5
    pool = frames_of(f, s, p, seed=9)
    idx = torch.tensor([[0, -1, 3], [f, 2, -1], [1, 2, 3]], dtype=torch.int32)        # -1 and F: missing
    crop = torch.tensor([[0, 2], [2, 1], [1, 1]], dtype=torch.int32)
    lut = normalize_lut()
    n = idx.numel() * p * s * s
    buf, out, guard = guarded(n, (3, 3, p, s, s), out_dtype)
    hip.u8_pool_gather_crop(pool.to(DEV), idx.to(DEV), lut.to(DEV), 127, crop.to(DEV), 1, out, 0, p)(stream())
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, DevicePreprocess(DEV, hip, out_dtype)(materialise(pool, idx), crop).cpu())
    fv = lut[127].to(out_dtype)
    assert bool((got[0, 1, :, 1:, :s - 1] == fv).all()) and not got[0, 1, :, 0].any() and not got[0, 1, :, :, s - 1].any()
    assert bool((got[1, 0, :, :s - 1] == fv).all()) and not got[1, 0, :, s - 1].any()
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("s,p", [(13, 5), (16, 21)])
def test_crop_values_far_outside_their_range_are_safe(hip, s, p, out_dtype):
    pad = 1
    pool = frames_of(4, s, p, seed=11)
    idx = torch.tensor([[0, 1], [2, 3], [3, -1], [1, 0], [2, 2], [0, 3], [1, 1], [3, 3]], dtype=torch.int32)
    crop = torch.tensor([[-50, 1], [1, 10 ** 6], [-(2 ** 31), 2 ** 31 - 1], [s + 2 * pad + 5, 0], [2 ** 31 - 1, -(2 ** 31)],
                         [pad + 3, pad - 2], [pad - (s - 1), pad + (s - 1)], [pad, pad - s]], dtype=torch.int32)
    n = idx.numel() * p * s * s
    buf, out, guard = guarded(n, (8, 2, p, s, s), out_dtype)
    hip.u8_pool_gather_crop(pool.to(DEV), idx.to(DEV), normalize_lut().to(DEV), 127, crop.to(DEV), pad, out, 0, p)(stream())
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, pool_gather_crop(pool, idx, normalize_lut(), 127, crop, pad, 0, p).to(out_dtype))
    assert not got[:5].any() and not got[7].any() and got[5].any() and got[6].any()   # one pixel of [6] is inside: a corner
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())


def test_two_runs_are_bit_equal(hip):
    f, s, p, rows = SHAPES["pad_of_4"]
    pool, idx = frames_of(f, s, p, seed=1).to(DEV), torch.tensor(rows, dtype=torch.int32)
    crop = crops_of(4)[-1]
    assert torch.equal(gather_crop(hip, pool, idx, crop, 4, torch.bfloat16), gather_crop(hip, pool, idx, crop, 4, torch.bfloat16))


def test_captured_graph_follows_new_indices_and_crops(hip):
    pool = frames_of(6, 16, 21, seed=4)
    pd, lut = pool.to(DEV), normalize_lut().to(DEV)
    idx = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5]], dtype=torch.int32).to(DEV)
    crop = torch.tensor([[1, 1], [0, 2]], dtype=torch.int32).to(DEV)
    out = torch.empty(2, 4, 21, 16, 16, device=DEV)
    run = hip.u8_pool_gather_crop(pd, idx, lut, 127, crop, 1, out)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(stream())
    for rows, offs in (([[5, 4, 3, 2], [1, 1, -1, 0]], [[2, 0], [0, 0]]), ([[3, 3, 3, 3], [6, 0, 5, 2]], [[0, 1], [-3, 40]])):
        new, newc = torch.tensor(rows, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32)
        idx.copy_(new)
        crop.copy_(newc)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), pool_gather_crop(pool, new, normalize_lut(), 127, newc, 1, 0, 21)), rows


# ------------------------------------------------------------------ ResidentTrainSet and the Trainer
def _cfg(tmp_path, jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.R3D_INPUT = KEY                                # 64 x 64 crops
    cfg.MODEL.NAME = "slowfast-test"
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


def _clip_frames(item, hip):
    """(T, S, S, 21) uint8 frames of a video_item over a clip's indices, a missing frame as bytes of 127"""
    if KEY + "_rawpool" in item:
        hw = item["raw_hw"]
        frames = PadResize(64, DEV, hip)(item[KEY + "_rawpool"], raw_offsets(hw, 21), hw).cpu()
        item = {KEY + "_pool": frames, "windows": item["windows"], "label": item["label"]}
    return unpool_item(item)[0][KEY + "_u8"]


@pytest.mark.parametrize("kind,half", [("as_uint8", False), ("as_uint8", True), ("raw", True)])
def test_resident_train_set_on_the_device_equals_its_replayed_plan(hip, tmp_path, kind, half):
    from video_classification_amd.train import SyntheticChalearn, jitter_ranges
    cfg = _cfg(tmp_path, jitter=True)
    ds = SyntheticChalearn(cfg, "train", num_videos=6, seed=3, frames_per_video=(2, 9), raw_side=(20, 40), **{kind: True})
    assert min(ds.vframes) < 4 < max(ds.vframes)
    cap = sum(ds.vframes) // 2 + 8 if half else 200
    r = ResidentTrainSet(ds, cfg, DEV, hip, batch_size=2, drop_last=True, seed=5, capacity_frames=cap, jitter=jitter_ranges(cfg))
    pre, uploaded = DevicePreprocess(DEV, hip), []
    for e in range(2):
        plan, before = r.plan(e), r.bytes_uploaded
        got = list(r.epoch(e))
        torch.cuda.synchronize()
        assert len(got) == len(plan) == 3
        for batch, (videos, indices, crop, jitter) in zip(got, plan):
            assert batch[KEY].device.type == "cuda" and batch[KEY].dtype == torch.float32
            assert batch["label"].tolist() == [ds.label(v) for v in videos] and torch.equal(batch["jitter"], jitter)
            frames = torch.stack([_clip_frames(ds.video_item(v, indices[n].tolist()), hip) for n, v in enumerate(videos)])
            assert torch.equal(batch[KEY].cpu(), pre(frames, crop).cpu())
        uploaded.append(r.bytes_uploaded - before)
        assert r.spill_peak <= 8 and sum(r.pool.live.values()) == r.resident_frames
    item_bytes = lambda v, ks=None: sum(t.numel() for k, t in ds.video_item(v, ks).items() if k in (KEY + "_pool", KEY + "_rawpool"))
    resident = sorted(v for v, ok in r._resident.items() if ok)
    if not half:
        assert resident == list(range(6)) and uploaded == [sum(item_bytes(v) for v in range(6)), 0] and r.spilled_clips == 0
    else:
        assert 0 < len(resident) < 6 and r.spilled_clips == 6 - len(resident)
        spilled = [(v, sorted(set(row.tolist()))) for vs, idx, _, _ in r.plan(1) for v, row in zip(vs, idx) if v not in resident]
        assert uploaded[1] == sum(item_bytes(v, ks) for v, ks in spilled) > 0


def test_trainer_train_epoch_from_the_resident_set(hip, tmp_path):
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = _cfg(tmp_path)
    cfg.DEBUG = True
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 100 * FRAME / 2 ** 30
    tr = SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True, frames_per_video=(3, 8))
    te = SyntheticChalearn(cfg, "test", num_videos=2, seed=2, pooled=True, frames_per_video=(3, 6))
    trainer = Trainer(cfg, train_set=tr, test_set=te, device=DEV, backend=hip)
    assert trainer.resident.capacity == 100
    seen = []
    prepare = trainer.mm.prepare_data
    trainer.mm.prepare_data = lambda batch: (seen.append(batch), prepare(batch))[1]
    loss, _ = trainer.train_epoch()
    torch.cuda.synchronize()
    first = trainer.resident.plan(0)[0]
    assert math.isfinite(loss) and len(seen) == 1                             # DEBUG: one step
    assert sorted(seen[0]) == [KEY, "label"] and tuple(seen[0][KEY].shape) == (2, 4, 21, 64, 64)
    assert seen[0]["label"].tolist() == [tr.label(v) for v in first[0]]
    assert trainer.resident.bytes_uploaded == sum(tr.vframes[v] for v in first[0]) * FRAME
