"""sfk_roi_resize_warp / _pool_warp / _ragged_warp on an MI355X (include/sfk_roi_warp.h): every comparison is bit for bit
(torch.equal) against roi_warp32 (tests/ref_roi_warp.py), the contract in float32 torch ops, in f32 and bf16, into a framed
destination (sentinel planes, rows and columns around what the launch may write, c_off = 1).  The cases are ref_roi_warp's --
the ones the CPU test proves six mutants of the emulation are refused by: 40 x 56 x 7 sources with padded strides; output
sizes one below, at and above the tile and a tall one; a 3x downscaling, an upscaling, an extent-equals-S, a 1-pixel-wide, a
corner-touching and a beyond-the-frame box, each in both antialias modes; identity, corner crops, flip, transpose, half-pixel
shifts, wide random draws, a minifying row, far-out rows; and a 64 x 96 box whose window exceeds the staging budget, so the
taps come from global memory.  Then: integer-translation rows against the sibling launch with crop on the same memory; the
three sources on the same clips; the float64 bound; a captured launch following its table; one v2 train step.  No non-finite
matrix is launched here: the no-load rule for those is covered by the emulation, validate_warp_rows and code review."""
import pytest
import torch

import ref_roi_warp as R
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import byte_lut, draw_affine

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
CASES = R.all_cases()


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_kernel_is_roi_warp32_bit_for_bit(hip, name, out_dtype):
    case = CASES[name]
    got = R.check_case(hip, DEV, name, case, out_dtype)
    where = case["where"]
    if where:
        assert got[where["identity"][0]].any() and got[where["draws"][1]].any()      # (not a comparison of zeros with zeros)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_the_three_sources_agree_bit_for_bit(hip, out_dtype):
    R.check_sources(hip, DEV, out_dtype)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith(("box_", "global_"))])
def test_the_kernel_is_within_the_derived_bound_of_float64(hip, name):
    R.check_f64(hip, DEV, name, CASES[name])


@pytest.mark.parametrize("antialias", [False, True], ids=["aa0", "aa1"])
@pytest.mark.parametrize("out_dtype", DTYPES, ids=["f32", "bf16"])
def test_integer_translation_rows_equal_the_sibling_launch_with_crop(hip, out_dtype, antialias):
    """ties the new kernel to the three shipped ones on the same memory, with no reference in between"""
    case = R.source_case(antialias)
    oh, ow = case["out_h"], case["out_w"]
    n, t = case["index"].shape
    lut = byte_lut().to(DEV)
    src, pool, arena = case["src"].to(DEV), case["pool"].to(DEV), case["arena"].to(DEV)
    index, offset, hw = case["index"].to(DEV), case["offset"].to(DEV), case["hw"].to(DEV)
    box, rbox = case["box"].to(DEV), case["ragged_box"].to(DEV)
    pad = ow // 10
    for top, left in [(0, 0), (0, 2 * pad), (2 * pad, 0), (2 * pad, 2 * pad), (pad, pad), (pad + 1, pad - 1)]:
        crop = torch.tensor([[top, left], [2 * pad - top, 2 * pad - left]], dtype=torch.int32).to(DEV)
        rows = torch.tensor([[1.0, 0.0, l - pad, 0.0, 1.0, tt - pad] for tt, l in crop.tolist()]).to(DEV)
        want = [torch.empty(n, t, R.C, oh, ow, dtype=out_dtype, device=DEV) for _ in range(3)]
        got = [torch.empty_like(w) for w in want]
        hip.roi_resize(src, lut, box, want[0], antialias, crop, pad)(stream())
        hip.roi_resize_warp(src, lut, box, rows, got[0], antialias)(stream())
        hip.roi_resize_pool(pool, index, lut, R.FILL, box, want[1], antialias, crop, pad, c0=case["c0"], c=R.C)(stream())
        hip.roi_resize_pool_warp(pool, index, lut, R.FILL, box, rows, got[1], antialias, c0=case["c0"], c=R.C)(stream())
        hip.roi_resize_ragged(arena, offset, hw, lut, R.FILL, rbox, want[2], antialias, crop, pad, pitch=R.C, max_hw=(R.H, R.W))(stream())
        hip.roi_resize_ragged_warp(arena, offset, hw, lut, R.FILL, rbox, rows, got[2], antialias, pitch=R.C, max_hw=(R.H, R.W))(stream())
        torch.cuda.synchronize()
        for kind, g, w in zip(("stacked", "pool", "ragged"), got, want):
            assert bool(w.any()) and torch.equal(g, w), (kind, top, left)


def test_a_box_whose_extent_equals_the_output_equals_the_sibling_launch(hip):
    """the in == out shortcut the sibling takes and this kernel dropped"""
    oh, ow = R.BOX_SIZE
    rows_l, tl, pad = R.crop_rows(oh, ow)
    n = len(rows_l)
    src = R.random_clip(n, 2, seed=3).to(DEV)
    x1, y1 = 7, 9
    box = torch.tensor([[x1, y1, x1 + ow, y1 + oh]] * n, dtype=torch.int32).to(DEV)
    lut = byte_lut().to(DEV)
    for aa in (False, True):
        want = torch.empty(n, 2, R.C, oh, ow, device=DEV)
        got = torch.empty_like(want)
        hip.roi_resize(src, lut, box, want, aa, torch.tensor(tl, dtype=torch.int32).to(DEV), pad)(stream())
        hip.roi_resize_warp(src, lut, box, torch.tensor(rows_l).to(DEV), got, aa)(stream())
        torch.cuda.synchronize()
        assert bool(want.any()) and torch.equal(got, want), aa


def test_a_captured_launch_follows_its_warp_table(hip):
    """captured once; the table rewritten in place; replayed twice; each replay against roi_warp32"""
    oh, ow = 17, 33
    src_h = R.random_clip(2, 2, seed=9)
    src = torch.empty_strided(src_h.shape, src_h.stride(), dtype=torch.uint8, device=DEV)
    src.copy_(src_h)
    lut = byte_lut().to(DEV)
    box_h = torch.tensor([[3, 2, 50, 37], [20, 15, 29, 21]], dtype=torch.int32)
    box = box_h.to(DEV)
    g = torch.Generator().manual_seed(10)
    wild = dict(degrees=30.0, scale=(0.6, 1.6), shear=10.0, flip=0.5)
    table = draw_affine(2, ow, ow // 10, generator=g, **wild).to(DEV)
    out = torch.empty(2, 2, R.C, oh, ow, device=DEV)
    run = hip.roi_resize_warp(src, lut, box, table, out, True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(side.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(stream())
    for k in range(2):
        new = draw_affine(2, ow, ow // 10, generator=g, **wild) if k == 0 else torch.tensor([[2.5, 0.3, -4.0, -0.3, 2.5, -2.0],
                                                                                              [1.0, 0.0, -2.0, 0.0, 1.0, 3.0]])
        table.copy_(new.to(DEV))
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        want = R.roi_warp32(src_h, byte_lut(), box_h, new, oh, ow, True)
        assert bool(want.any()) and torch.equal(out.cpu(), want), k


def test_one_v2_train_step_from_a_warp_batch_and_from_a_resident_affine_batch(hip):
    """mini model (depth 18, head pools (1, 1, 1) / (4, 1, 1)), N 2, T 4, S 32, eager: prepare_data samples the uint8 batch
    through its 'warp' rows, ResidentGestureSet(affine=) gathers its own; the clip handed to the step is roi_warp32's of the
    same frames, boxes and rows, bit for bit, and the step's loss is finite"""
    import math

    from video_classification_amd import arch
    from video_classification_amd import gesture_v2 as v2
    from video_classification_amd import train as v1
    from video_classification_amd.config import get_cfg
    from video_classification_amd.input_pipeline import ResidentGestureSet
    from video_classification_amd.slowfast import SlowFast
    cfg = get_cfg()
    cfg.CHALEARN.ROOT, cfg.CHALEARN.BATCH_SIZE, cfg.CHALEARN.CLIP_LEN, cfg.CHALEARN.NUM_CLASS = "/nonexistent", 2, 4, 7
    cfg.MODEL.NAME, cfg.MODEL.INPUT_SIZE, cfg.MODEL.DEPTH, cfg.MODEL.AFFINE, cfg.NUM_CPU = "gesture-v2", 32, 18, True, 0
    s, h, w = 32, 48, 64
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((1, 1, 1), (4, 1, 1)))
    torch.manual_seed(0)
    model = SlowFast(spec, dtype=torch.float32, device=DEV)
    model.train()
    step = v1.TrainStep(model.engine, lr=1e-3, use_graph=False, optimizer="sgd", momentum=0.9)
    mm = v2.ModelManager(cfg, DEV, hip)
    ds = v2.SyntheticGesture(cfg, "train", num_videos=2, seed=3, h=h, w=w, min_box=8, videos=True, frames_per_video=(5, 8))
    # the loader route: a collated batch of two train items, each with its own 'warp' row
    items = [ds[0], ds[1]]
    batch = {k: torch.stack([torch.as_tensor(it[k]) for it in items]) for k in ("frames_u8", "box", "warp", "label")}
    assert batch["warp"].dtype == torch.float32 and tuple(batch["warp"].shape) == (2, 6)
    x, y = mm.prepare_data(batch)
    want = R.roi_warp32(batch["frames_u8"], byte_lut(), batch["box"], batch["warp"], s, s, True).permute(0, 2, 1, 3, 4)
    assert bool(want.any()) and torch.equal(x[0].cpu(), want[:, 0:5]) and torch.equal(x[1].cpu(), want[:, 5:7])
    loss = float(step(x[0], x[1], y))
    assert math.isfinite(loss)
    # the resident route
    rs = ResidentGestureSet(ds, cfg, DEV, hip, batch_size=2, seed=1, capacity_frames=40, affine=v1.affine_ranges(cfg))
    (entry,) = rs.plan(0)
    (rb,) = list(rs.epoch(0))
    stacked = torch.stack([ds.video_item(v, entry[1][n].tolist())["frames_pool"] for n, v in enumerate(entry[0])])
    want = R.roi_warp32(stacked, byte_lut(), entry[2], entry[3], s, s, True)
    assert entry[3].dtype == torch.float32 and bool(want.any()) and torch.equal(rb["clip_v2"].cpu(), want)
    x, y = mm.prepare_data(rb)
    loss = float(step(x[0], x[1], y))
    torch.cuda.synchronize()
    assert math.isfinite(loss)
