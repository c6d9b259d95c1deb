"""sfk_u8_pool_gather on an MI355X (include/sfk_pool.h): bit-exactness against sfk_u8_normalize_crop (DevicePreprocess) on the
materialised clips, in f32 and bf16, for aligned and never-aligned rows, a pixel pitch wider than the channels read, repeated and
out-of-order indices and a single slab; missing frames and untouched memory around the output; a pool whose last frame lies
beyond byte 2^31; reproducibility; a captured graph following new indices; and Trainer.run_eval on pooled videos against the
same videos as lists of uint8 clips.  Both sides are table lookups of the same bytes through the same table, so every
comparison is torch.equal."""
import numpy as np
import pytest
import torch

from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import DevicePreprocess, FramePool, normalize_lut, uniform_windows, unpool_item

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


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


def gather(hip, pool_dev, idx, out_dtype, fill=127, c0=0, c=None):
    f, h, w, p = pool_dev.shape
    c = p - c0 if c is None else c
    out = torch.empty(idx.shape[0], idx.shape[1], c, h, w, dtype=out_dtype, device=DEV)
    hip.u8_pool_gather(pool_dev, idx.to(DEV), normalize_lut().to(DEV), fill, out, c0, c)(stream())
    torch.cuda.synchronize()
    return out.cpu()


CASES = {
    # name -> (F, S, P, index rows)
    "two_windows_and_a_wrapped_one": (11, 40, 21, uniform_windows(11, 4).tolist() + [[i % 11 for i in range(9, 13)]]),
    "rows_of_65_bytes": (5, 13, 5, [[0, 1, 2], [2, 3, 4]]),
    "repeated_and_out_of_order": (6, 16, 21, [[5, 5, 5, 5], [3, 0, 4, 1], [0, 5, 0, 5]]),
    "one_slab": (3, 24, 21, [[2]]),
}


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_gather_is_bit_identical_to_normalize_crop_of_the_materialised_clips(hip, name, out_dtype):
    f, s, p, rows = CASES[name]
    pool = frames_of(f, s, p, seed=len(name))
    idx = torch.tensor(rows, dtype=torch.int32)
    want = DevicePreprocess(DEV, hip, out_dtype)(materialise(pool, idx)).cpu()
    got = gather(hip, pool.to(DEV), idx, out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == (idx.shape[0], idx.shape[1], p, s, s)
    assert torch.equal(got, want)
    assert torch.equal(got, normalize_lut()[materialise(pool, idx).long()].permute(0, 1, 4, 2, 3).to(out_dtype))


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_pixel_pitch_wider_than_the_channels_read(hip, out_dtype):
    pool = frames_of(5, 13, 8, seed=3)                                        # pitch 8, channels 1..5 read
    idx = torch.tensor([[4, 0, 2], [1, 1, 3]], dtype=torch.int32)
    want = DevicePreprocess(DEV, hip, out_dtype)(materialise(pool, idx)[..., 1:6].contiguous()).cpu()
    assert torch.equal(gather(hip, pool.to(DEV), idx, out_dtype, c0=1, c=5), want)
    # the same bytes as a strided view of a wider buffer: the strides come from the tensor
    wide = torch.zeros(5, 13, 16, 8, dtype=torch.uint8)
    wide[:, :, :13] = pool
    assert torch.equal(gather(hip, wide.to(DEV)[:, :, :13], idx, out_dtype, c0=1, c=5), want)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("fill", [127, 0])
def test_missing_frames_and_untouched_memory(hip, fill, out_dtype):
    f, s, p, guard = 4, 13, 5, 64
    pool = frames_of(f, s, p, seed=9)
    idx = torch.tensor([[0, -1, 3], [f, 2, -1], [1, 2, 3]], dtype=torch.int32)        # -1 and F: missing
    lut = normalize_lut()
    n = idx.numel() * p * s * s
    buf = torch.full((n + 2 * guard,), -7.0, dtype=out_dtype, device=DEV)
    out = buf[guard:guard + n].view(3, 3, p, s, s)
    assert out.data_ptr() % 16 == 0
    hip.u8_pool_gather(pool.to(DEV), idx.to(DEV), lut.to(DEV), fill, out, 0, p)(stream())
    torch.cuda.synchronize()
    got = out.cpu()
    for (i, j) in [(0, 1), (1, 0), (1, 2)]:
        assert torch.equal(got[i, j], torch.full((p, s, s), float(lut[fill])).to(out_dtype)), (i, j)
    want = lut[materialise(pool, idx, fill).long()].permute(0, 1, 4, 2, 3).to(out_dtype)
    assert torch.equal(got, want)                                             # the neighbours are what they are without them
    assert torch.equal(got[2], DevicePreprocess(DEV, hip, out_dtype)(pool[None, 1:4]).cpu()[0])
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())


def test_pool_larger_than_2_31_bytes(hip):
    frame_stride = 1_090_000_005                                              # not a multiple of 16 either
    try:
        big = torch.empty(2 * frame_stride + 16 * 16 * 5, dtype=torch.uint8, device=DEV)
    except RuntimeError as e:                                                 # torch.OutOfMemoryError is one
        pytest.skip(f"no room for a 2.2 GB pool on this device: {str(e)[:80]}")
    view = big.as_strided((3, 16, 16, 5), (frame_stride, 80, 5, 1))
    assert view[2].data_ptr() - big.data_ptr() > 2 ** 31
    pool = frames_of(3, 16, 5, seed=31)
    view.copy_(pool.to(DEV))                                                  # only those three frames are written
    idx = torch.tensor([[2, 0, 1], [1, 2, 2]], dtype=torch.int32)
    want = DevicePreprocess(DEV, hip)(materialise(pool, idx)).cpu()
    assert torch.equal(gather(hip, view, idx, torch.float32), want)
    del view, big
    torch.cuda.empty_cache()


def test_two_runs_are_bit_equal(hip):
    f, s, p, rows = CASES["two_windows_and_a_wrapped_one"]
    pool, idx = frames_of(f, s, p, seed=1).to(DEV), torch.tensor(rows, dtype=torch.int32)
    assert torch.equal(gather(hip, pool, idx, torch.bfloat16), gather(hip, pool, idx, torch.bfloat16))


def test_captured_graph_follows_new_indices(hip):
    pool = frames_of(6, 16, 21, seed=4)
    pd, lut = pool.to(DEV), normalize_lut().to(DEV)
    first = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5]], dtype=torch.int32)
    idx = first.to(DEV)
    out = torch.empty(2, 4, 21, 16, 16, device=DEV)
    run = hip.u8_pool_gather(pd, idx, lut, 127, out)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(stream())
    for rows in ([[5, 4, 3, 2], [1, 1, -1, 0]], [[3, 3, 3, 3], [6, 0, 5, 2]]):
        new = torch.tensor(rows, dtype=torch.int32)
        idx.copy_(new)
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), normalize_lut()[materialise(pool, new).long()].permute(0, 1, 4, 2, 3)), rows


def test_frame_pool_on_the_device(hip):
    """videos of 3, 11 and 25 frames in batches of three windows: one upload per frame, every clip DevicePreprocess's"""
    T, bs = 4, 3
    videos = [frames_of(f, 24, 21, seed=f) for f in (3, 11, 25)]
    pool, refs, want, got = FramePool(DEV, hip), [], [], []
    for v in videos:
        win = uniform_windows(len(v), T)
        base = pool.add(v, win)
        video = {"base": base, "rows": pool.rows(base, win), "left": len(win)}
        refs += [(video, r) for r in range(len(win))]
        want.append(v[win.long()])
    while refs:
        batch, refs = refs[:bs], refs[bs:]
        got.append(pool.gather(torch.stack([v["rows"][r] for v, r in batch])))
        for v, _ in batch:
            v["left"] -= 1
            if v["left"] == 0:
                pool.release(v["base"])
    torch.cuda.synchronize()
    assert pool.bytes_uploaded == sum(v.numel() for v in videos) == (3 + 11 + 25) * 24 * 24 * 21 and not pool.live
    assert torch.equal(torch.cat(got).cpu(), DevicePreprocess(DEV, hip)(torch.cat(want)).cpu())


class _Unpooled(torch.utils.data.Dataset):
    def __init__(self, pooled_set):
        self.s = pooled_set

    def __len__(self):
        return len(self.s)

    def __getitem__(self, i):
        return unpool_item(self.s[i])


def test_trainer_pooled_run_eval_equals_the_unpooled_one(hip, tmp_path):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.R3D_INPUT = "CropLHand"                       # 64 x 64 crops
    cfg.MODEL.NAME = "slowfast-test"
    cfg.DEBUG = True
    tr_set = SyntheticChalearn(cfg, "train", num_videos=2, seed=1, as_uint8=True)
    te_set = SyntheticChalearn(cfg, "test", num_videos=3, seed=2, pooled=True, frames_per_video=(3, 14))
    assert sum(te_set.nclips) > 2 and max(te_set.nclips) >= 2
    loader = torch.utils.data.DataLoader(tr_set, batch_size=2, shuffle=False, drop_last=True)
    pooled = torch.utils.data.DataLoader(te_set, batch_size=2, shuffle=False, collate_fn=lambda x: x)
    flat = torch.utils.data.DataLoader(_Unpooled(te_set), batch_size=2, shuffle=False, collate_fn=lambda x: x)
    trainer = Trainer(cfg, train_loader=loader, test_loader=pooled, device=DEV, backend=hip)
    a, b = trainer.run_eval(flat), trainer.run_eval(flat)
    spread = float(np.abs(a["ps"] - b["ps"]).max())        # run to run, unpooled
    got = trainer.run_eval()
    err = float(np.abs(got["ps"] - a["ps"]).max())
    print(f"pooled run_eval: |ps - unpooled| {err:.3e}, unpooled run-to-run {spread:.3e}")
    assert got["sv"] == a["sv"] == te_set.nclips
    assert np.array_equal(got["t"], a["t"]) and got["acc"] == a["acc"]
    assert err <= spread
    assert trainer.frame_pool.bytes_uploaded == sum(te_set[i]["CropLHand_pool"].numel() for i in range(len(te_set)))
    assert not trainer.frame_pool.live
