"""sfk_u8_pool_gather_warp on an MI355X (include/sfk_warp.h): every comparison is bit for bit (torch.equal) against warp32
(tests/ref_warp.py), the contract in float32 torch ops, in f32 and bf16, with sentinels around `out`.  The cases are
ref_warp's -- the ones the CPU test proves five mutants of the emulation are refused by: a pool with padded strides, every
channel range, index tables with a repeated frame, a -1 and an index >= frames, index = NULL; extents one below, at and above
the tile, non-square, 16-byte and element-wise stores; identity, corner crops, flip, transpose, half-pixel shifts, random
draws, far-out rows and a minifying row that takes the global-tap path.  Then: integer-translation rows against a
sfk_u8_pool_gather_crop launch on the same pool; S 192 with the frames above 2^31 bytes of a pool; a captured launch following
its table; and one TrainStep from a 'warp' batch against the float clip warp32 produced.  No non-finite matrix is used here:
the no-load rule for those is covered by the emulation, the host-side validate and code review."""
import pytest
import torch

import ref_warp as R
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import affine_inverse, draw_affine, identity_warp_rows, normalize_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
CASES = R.all_cases()
WILD = dict(degrees=30.0, scale=(0.6, 1.6), shear=10.0, flip=0.5)


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def stream():
    return torch.cuda.current_stream().cuda_stream


def on_device(pool):
    """the pool on the device with the strides it has on the host (a padded view moves with its padding)"""
    base = pool._base if pool._base is not None else pool
    return base.to(DEV).as_strided(tuple(pool.shape), pool.stride(), pool.storage_offset())


def guarded(shape, out_dtype, guard=64):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), -7.0, dtype=out_dtype, device=DEV)
    out = buf[guard:guard + n].view(shape)
    assert out.data_ptr() % 16 == 0
    return buf, out, guard, n


def gpu_gather(hip):
    def gather(pool, index, lut, fill, warp, c0, c, out_dtype):
        n, t = pool.shape[:2] if index is None else index.shape
        h, w = pool.shape[-3:-1]
        buf, out, guard, numel = guarded((n, t, c, h, w), out_dtype)
        hip.u8_pool_gather_warp(on_device(pool), None if index is None else index.to(DEV), lut.to(DEV), fill,
                                warp.to(DEV).contiguous(), out, c0, c)(stream())
        torch.cuda.synchronize()
        assert bool((buf[:guard] == -7).all()) and bool((buf[guard + numel:] == -7).all()), "a sentinel around out was written"
        return out.cpu()
    return gather


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_kernel_is_warp32_bit_for_bit(hip, name, out_dtype):
    case = CASES[name]
    got = R.check(gpu_gather(hip), case, out_dtype)
    where = case.get("where")
    if where:
        assert got[where["identity"][0]].any() and got[where["draws"][1]].any()      # (not a comparison of zeros with zeros)


def test_the_minifying_row_takes_the_global_taps_where_the_frame_exceeds_the_budget(hip):
    """the host-side predicate of the binding, from the matrix alone: it neither times nor inspects the kernel"""
    h, w = R.EXTENTS[-1]
    assert (h, w) == (48, 40)
    assert hip.warp_fallback_tiles(h, w, 21, 21, R.MINIFY) > 0 and hip.warp_fallback_tiles(h, w, 21, 21, identity_warp_rows(1)[0]) == 0
    warp, where = R.matrix_rows(h, w, seed=len(R.EXTENTS) - 1)
    assert warp[where["minify"][0]].tolist() == R.MINIFY
    assert hip.warp_fallback_tiles(h, w, 21, 21, warp[where["minify"][1]].tolist()) > 0        # and the rotated one
    assert all(hip.warp_fallback_tiles(h, w, 21, 21, warp[k].tolist()) == 0 for k in where["crop"] + where["flip"] + where["far"])
    for hh, ww in R.EXTENTS[:-1]:                      # a frame that fits the budget whole is always staged
        assert hip.warp_fallback_tiles(hh, ww, 21, 21, R.MINIFY) == 0


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("h,w", [(24, 40), (17, 33)], ids=["16_byte_stores", "element_stores"])
def test_integer_translation_rows_equal_a_crop_launch_on_the_same_pool(hip, h, w, out_dtype):
    """ties the new kernel to the shipped one, with no reference in between"""
    pad = w // 10
    pool = on_device(R.random_pool(4, h, w, seed=7, row_pad=5, frame_pad=3))
    index = torch.tensor([[0, 3, -1], [2, 2, 4]], dtype=torch.int32).to(DEV)
    lut = normalize_lut().to(DEV)
    for c0, c in [(0, 21), (5, 15)]:
        for top, left in [(0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad), (pad, pad), (pad + 1, pad - 1)]:
            crop = torch.tensor([[top, left], [2 * pad - top, 2 * pad - left]], dtype=torch.int32)
            rows = torch.tensor([[1.0, 0.0, l - pad, 0.0, 1.0, t - pad] for t, l in crop.tolist()])
            want = torch.empty(2, 3, c, h, w, dtype=out_dtype, device=DEV)
            got = torch.empty_like(want)
            hip.u8_pool_gather_crop(pool, index, lut, 127, crop.to(DEV), pad, want, c0, c)(stream())
            hip.u8_pool_gather_warp(pool, index, lut, 127, rows.to(DEV), got, c0, c)(stream())
            torch.cuda.synchronize()
            assert torch.equal(got, want) and got.any(), (c0, c, top, left)


@pytest.fixture(scope="module")
def big():
    """S 192, T 4, N 2: five frames, their table, one row of the config defaults (staged) and one that minifies 2x under 30 degrees
    (global taps), and warp32 of them
    (computed once for both dtypes)"""
    s = 192
    frames = torch.randint(0, 256, (5, s, s, 21), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    local = torch.tensor([[0, 1, 2, 3], [4, 4, -1, 0]], dtype=torch.int32)
    g = torch.Generator().manual_seed(4)
    strong = affine_inverse(s, s // 10, 25, 10, angle=30.0, scale=0.5, shear=10.0, flipped=True).reshape(1, 6).float()
    warp = torch.cat([draw_affine(1, s, s // 10, 10.0, (0.85, 1.15), generator=g), strong])
    return frames, local, warp, R.warp32(frames, local, normalize_lut(), 127, warp)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_s192_with_the_frames_above_2_31_bytes_of_the_pool(hip, big, out_dtype):
    """The largest shape.  The arena is allocated, not filled (2.2 GB of address space, no traffic): only the five frames the
    table names are written, at slots whose byte offset frame_stride * index is above 2^31, where 32-bit offset arithmetic
    would read elsewhere."""
    frames, local, warp, want = big
    s, frame = 192, 192 * 192 * 21
    first = (2 ** 31) // frame + 2
    arena = torch.empty(first + 5, s, s, 21, dtype=torch.uint8, device=DEV)
    assert first * frame > 2 ** 31
    arena[first:].copy_(frames.to(DEV))
    assert hip.warp_fallback_tiles(s, s, 21, 21, warp[0].tolist()) == 0 < hip.warp_fallback_tiles(s, s, 21, 21, warp[1].tolist())
    buf, out, guard, numel = guarded((2, 4, 21, s, s), out_dtype)
    index = torch.where(local < 0, local, local + first)
    hip.u8_pool_gather_warp(arena, index.to(DEV), normalize_lut().to(DEV), 127, warp.to(DEV), out)(stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want.to(out_dtype))
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + numel:] == -7).all())


def test_a_captured_launch_follows_its_warp_table(hip):
    """captured once; the table rewritten in place; replayed twice; each replay against an eager launch"""
    h, w = 48, 40
    pool = R.random_pool(4, h, w, seed=9)
    pd, lut = on_device(pool), normalize_lut().to(DEV)
    index = torch.tensor([[0, 1, 2], [3, -1, 1]], dtype=torch.int32).to(DEV)
    g = torch.Generator().manual_seed(10)
    table = draw_affine(2, w, w // 10, generator=g, **WILD).to(DEV)
    out = torch.empty(2, 3, 21, h, w, device=DEV)
    run = hip.u8_pool_gather_warp(pd, index, lut, 127, table, out)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(side.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(stream())
    for k in range(2):
        new = draw_affine(2, w, w // 10, generator=g, **WILD) if k == 0 else torch.tensor([R.MINIFY, [1.0, 0.0, -2.0, 0.0, 1.0, 3.0]])
        table.copy_(new.to(DEV))
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = torch.empty_like(out)
        hip.u8_pool_gather_warp(pd, index, lut, 127, new.to(DEV), eager)(stream())
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out.cpu(), R.warp32(pool, index.cpu(), lut.cpu(), 127, new)), k


def test_one_train_step_from_a_warp_batch_equals_the_float_clip_of_warp32(hip):
    """depth 18, eager: prepare_data samples the uint8 batch through its 'warp' rows on the device; the same model fed the
    float clip warp32 produced, as a plain float batch, sees the same bits and reports the same loss"""
    from video_classification_amd import train as v1
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT, cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.NUM_CLASS = "/nonexistent", 2, 4, 7
    cfg.MODEL.NAME, cfg.MODEL.R3D_INPUT, cfg.MODEL.DEPTH, cfg.MODEL.AFFINE = "slowfast-LHand", "CropLHand", 18, True
    key = cfg.MODEL.R3D_INPUT
    mm = v1.ModelManager(cfg, DEV, hip)
    torch.manual_seed(0)
    model = mm.init_model()
    twin = mm.init_model()
    twin.load_state_dict(model.state_dict(), strict=True)
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (2, 4, 64, 64, 21), generator=g, dtype=torch.uint8)
    warp = draw_affine(2, 64, 6, *v1.affine_ranges(cfg), generator=g)
    labels = torch.tensor([1, 4])
    x, y = mm.prepare_data({key + "_u8": frames, "warp": warp, "label": labels})
    clip = R.warp32(frames, None, normalize_lut(), 127, warp)
    fx, fy = mm.prepare_data({key: clip, "label": labels})
    assert all(torch.equal(a, b) for a, b in zip(x, fx)) and x[0].shape[1] == 5 and x[1].shape[1] == 15
    model.train()
    twin.train()
    loss = float(v1.TrainStep(model.engine, lr=1e-3, use_graph=False)(x[0], x[1], y))
    want = float(v1.TrainStep(twin.engine, lr=1e-3, use_graph=False)(fx[0], fx[1], fy))
    torch.cuda.synchronize()
    assert loss == loss and loss == want, (loss, want)
