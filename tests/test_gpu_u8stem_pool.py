"""MODEL.POOL_STEM on an MI355X: the uint8 stems reading the frame pool through its index table (include/sfk_u8stem_pool.h)
against the stacked-frame uint8 stems (include/sfk_u8stem.h) on ``arena[index]`` with missing frames as the constant fill
image -- forward and BatchNorm partial sums bit-identical, filter gradient to fp32 rounding; pool offsets beyond 2^31 and 2^32
bytes; garbage crops beside canary bytes; a captured TrainStep replayed on new tables written into the same tensors; the
Trainer on the resident set and the pooled run_eval with POOL_STEM on and off."""
import pytest
import torch

from helpers import rel_err
from test_gpu_u8_stem import _crop, cosine, stem_weights
from video_classification_amd._lib import FMap, HipBackend, StemSrc, stem_kp
from video_classification_amd.input_pipeline import PoolClip, U8Clip, normalize_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 127


def stacked(arena, index, fill=FILL):
    """the (n, t, s, s, pitch) frames the index table names, clip by clip; a missing frame is the constant image of fill"""
    f = arena.shape[0]
    idx = index.long()
    miss = (idx < 0) | (idx >= f)
    out = arena[idx.clamp(0, f - 1)]                       # (a missing frame reads a frame of the arena here, then is replaced)
    out[miss] = fill
    return out


def compare(kind, arena, index, c0, c, dt, crop, pad, cout=64, seed=0, t_index=None, kt=1):
    """kind '3d' (sfk_u8pstem_conv_* against sfk_u8stem_conv_*) or '2d' (sfk_u8pstem2d_* against sfk_u8stem2d_*)"""
    be = HipBackend()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(seed)
    (n, t), s = index.shape, arena.shape[1]
    lut = normalize_lut().to(DEV)
    xs = U8Clip(stacked(arena, index), c0, c, crop, pad, lut)
    xp = PoolClip(arena, index, c0, c, crop, pad, lut, FILL)
    assert tuple(xp.shape) == tuple(xs.shape)
    ti = None if t_index is None else torch.tensor(t_index, dtype=torch.int32, device=DEV)
    kt_ = t if kind == "2d" else kt
    ss, sp = StemSrc(xs, ti, kt_), StemSrc(xp, ti, kt_)
    t_out = 1 if kind == "2d" else (t if ti is None else len(t_index))
    ho = (s - 1) // 2 + 1
    kp = stem_kp(c, kt_)
    w = stem_weights(cout, c, kt_, g).to(dt).to(DEV)
    y_s = FMap(torch.full((n * t_out * ho * ho * cout,), float("nan"), dtype=dt, device=DEV), n, t_out, ho, ho, cout)
    y_p = FMap(torch.full_like(y_s.buf, float("nan")), n, t_out, ho, ho, cout)
    sfwd, swgrad = (be.u8stem2d_fwd, be.u8stem2d_wgrad) if kind == "2d" else (be.u8stem_conv_fwd, be.u8stem_conv_wgrad)
    pfwd, pwgrad = (be.u8pstem2d_fwd, be.u8pstem2d_wgrad) if kind == "2d" else (be.u8pstem_conv_fwd, be.u8pstem_conv_wgrad)
    mt = be.u8stem_tiles(sp, y_p)
    assert mt == be.u8stem_tiles(ss, y_s)
    st_s, st_p = torch.zeros(mt * cout * 2, device=DEV), torch.full((mt * cout * 2,), float("nan"), device=DEV)
    sfwd(ss, w, y_s, st_s)(stream)
    pfwd(sp, w, y_p, st_p)(stream)
    dy = FMap((torch.randn(y_s.pixels * cout, generator=g) * 0.1).to(dt).to(DEV), n, t_out, ho, ho, cout)
    dw_s, dw_p = torch.zeros(cout * kp, device=DEV), torch.zeros(cout * kp, device=DEV)
    swgrad(ss, dy, dw_s)(stream)
    pwgrad(sp, dy, dw_p)(stream)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == torch.bfloat16 else torch.int32
    assert torch.isfinite(y_s.buf.float()).all() and float(y_s.buf.float().abs().max()) > 0
    assert torch.equal(y_p.buf.view(bits), y_s.buf.view(bits))                                 # bit-identical
    assert torch.equal(st_p.view(torch.int32), st_s.view(torch.int32))
    err = rel_err(dw_p, dw_s)
    print(f"{kind} c0 {c0} c {c} kt {kt_} {dt}: dw rel_err {err:.3e}")
    assert torch.isfinite(dw_p).all() and err < 1e-5
    return y_p


def pool_case(f, t, pitch, table, crop_mode, seed, s=64):
    """an arena of f random frames and an (n, t) table with a frame both clips share, a -1 and an index equal to f"""
    g = torch.Generator().manual_seed(seed)
    arena = torch.randint(0, 256, (f, s, s, pitch), generator=g, dtype=torch.uint8).to(DEV)
    index = torch.tensor(table, dtype=torch.int32)
    assert tuple(index.shape) == (2, t) and (index == -1).any() and (index == f).any()
    assert set(index[0].tolist()) & set(index[1].tolist()) - {-1, f}
    crop = _crop(crop_mode, 2, s // 10, g)
    return arena, index.to(DEV), None if crop is None else crop.to(DEV), s // 10


CROPS = [None, "random", "zero", "max"]
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@pytest.mark.parametrize("crop", CROPS)
@DTYPES
def test_pool_stem3d_cin5_kt1_gather(dt, crop):
    """PackPathway's t_index picks the frame first, the pool index is applied to the picked frame"""
    arena, index, crop, pad = pool_case(12, 8, 21, [[9, 3, 11, 0, 4, -1, 7, 12], [2, 2, 12, 6, 1, 9, 8, -1]], crop, 1)
    compare("3d", arena, index, 0, 5, dt, crop, pad, t_index=[0, 2, 5, 7], kt=1, seed=1)


@pytest.mark.parametrize("crop", CROPS)
@DTYPES
def test_pool_stem3d_cin15_c0_5(dt, crop):
    """the reference SlowFast's fast stem: channels 5:20, kt 1, cout 8"""
    arena, index, crop, pad = pool_case(9, 4, 21, [[8, -1, 3, 0], [3, 9, 5, 5]], crop, 2)
    compare("3d", arena, index, 5, 15, dt, crop, pad, cout=8, kt=1, seed=2)


@pytest.mark.parametrize("crop", CROPS)
@DTYPES
def test_pool_stem3d_kt3_missing_frames_beside_temporal_padding(dt, crop):
    """kt 3, channels 5:10: clip 0 has missing frames at both ends (the tap beyond them is temporal padding), clip 1 has
    one as a middle tap"""
    arena, index, crop, pad = pool_case(10, 5, 21, [[-1, 4, 7, 2, 10], [6, 4, -1, 10, 0]], crop, 4)
    compare("3d", arena, index, 5, 5, dt, crop, pad, cout=16, kt=3, seed=4)


@pytest.mark.parametrize("crop", CROPS)
@DTYPES
def test_pool_stem3d_generic_plane_path(dt, crop):
    """a channel count that is neither 5 nor 15 stages a plane at a time; kt 3 so that planes of three states mix (three
    channels: the patches of kt * c planes and the f32 filter rows have to fit in LDS together)"""
    arena, index, crop, pad = pool_case(8, 4, 21, [[5, 8, 1, -1], [-1, 1, 0, 7]], crop, 5)
    compare("3d", arena, index, 3, 3, dt, crop, pad, cout=16, kt=3, seed=5)


@pytest.mark.parametrize("crop", CROPS)
@DTYPES
@pytest.mark.parametrize("pitch", [21, 5])
def test_pool_stem2d_t10_c5(pitch, dt, crop):
    arena, index, crop, pad = pool_case(14, 10, pitch, [[13, 0, 5, 5, -1, 2, 14, 9, 1, 3], [4, 14, 5, 12, 11, -1, 6, 7, 8, 10]],
                                        crop, 3)
    compare("2d", arena, index, 0, 5, dt, crop, pad, seed=3)


BIG = 49940                                                # slots of (64, 64, 21): 4.296 GB
LOW, MID, HIGH = 0, 24967, 49935                           # slot MID is the first wholly above 2^31 bytes, HIGH lies above 2^32


@pytest.fixture(scope="module")
def big_arena():
    frame = 64 * 64 * 21
    assert BIG * frame > 2 ** 32 and (MID - 1) * frame < 2 ** 31 <= MID * frame and 2 ** 32 <= HIGH * frame
    arena = torch.empty((BIG, 64, 64, 21), dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(11)
    used = [LOW, LOW + 1, MID, MID + 1, HIGH, HIGH + 1, BIG - 1]
    for slot in used:                                      # only the frames the tables name are written
        arena[slot] = torch.randint(0, 256, (64, 64, 21), generator=g, dtype=torch.uint8).to(DEV)
    yield arena, used
    del arena
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,c0,c,cout,kt", [("3d", 0, 5, 64, 1), ("3d", 5, 15, 8, 1), ("3d", 3, 3, 16, 3), ("2d", 0, 5, 64, 4)])
def test_pool_offsets_beyond_32_bits(big_arena, kind, c0, c, cout, kt):
    """an arena of more than 2^32 bytes with frames in its first slot, just above 2^31 and just above 2^32 bytes"""
    arena, used = big_arena
    index = torch.tensor([[LOW, MID, HIGH, BIG - 1], [HIGH + 1, -1, MID + 1, BIG]], dtype=torch.int32)
    assert set(index.flatten().tolist()) - {-1, BIG} <= set(used) and int(index[0, 2]) * arena.stride(0) >= 2 ** 32
    g = torch.Generator().manual_seed(12)
    crop = _crop("random", 2, 6, g).to(DEV)
    compare(kind, arena, index.to(DEV), c0, c, torch.bfloat16, crop, 6, cout=cout, kt=kt, seed=12)


@pytest.mark.parametrize("kind,c0,c,kt", [("3d", 0, 5, 1), ("3d", 3, 3, 3), ("2d", 0, 5, 3)])
def test_pool_garbage_crops_beside_canaries(kind, c0, c, kt):
    """the arena is a slice of a larger buffer of canary bytes, the first and last frames are named, and the crop values lie far
    outside [0, 2*pad]: the output is the stacked clip's (no kernel writes the arena: a check of values only)"""
    g = torch.Generator().manual_seed(21)
    f, s, guard = 6, 64, 2
    buf = torch.full((f + 2 * guard, s, s, 21), 0xA5, dtype=torch.uint8, device=DEV)
    arena = buf[guard:guard + f]
    arena.copy_(torch.randint(0, 256, arena.shape, generator=g, dtype=torch.uint8))
    index = torch.tensor([[0, f - 1, -1], [f - 1, f, 0], [3, 0, f - 1]], dtype=torch.int32, device=DEV)
    crop = torch.tensor([[-(2 ** 31), 2 ** 31 - 1], [100000, -7], [40, 30]], dtype=torch.int32, device=DEV)
    before = buf.clone()
    lut = normalize_lut().to(DEV)
    be, stream = HipBackend(), torch.cuda.current_stream().cuda_stream
    n, t = index.shape
    kt_ = t if kind == "2d" else kt
    t_out, ho, cout = (1 if kind == "2d" else t), 32, 16
    w = stem_weights(cout, c, kt_, g).to(DEV)
    ys = []
    for x in (U8Clip(stacked(arena, index), c0, c, crop, 6, lut), PoolClip(arena, index, c0, c, crop, 6, lut, FILL)):
        y = FMap(torch.full((n * t_out * ho * ho * cout,), float("nan"), device=DEV), n, t_out, ho, ho, cout)
        fwd = {("3d", False): be.u8stem_conv_fwd, ("3d", True): be.u8pstem_conv_fwd, ("2d", False): be.u8stem2d_fwd,
               ("2d", True): be.u8pstem2d_fwd}[kind, isinstance(x, PoolClip)]
        fwd(StemSrc(x, None, kt_), w, y, None)(stream)
        ys.append(y)
    torch.cuda.synchronize()
    out = ys[1].view5()
    assert torch.equal(ys[1].buf.view(torch.int32), ys[0].buf.view(torch.int32))
    assert torch.equal(out[:2], torch.zeros_like(out[:2])) and float(out[2].abs().max()) > 0   # clips 0 and 1 lie outside their frames
    assert torch.equal(buf, before)


# ------------------------------------------------------------------ the whole path
def test_captured_train_step_follows_new_index_and_crop_tables():
    """TrainStep(use_graph=True) on a PoolClip; new index and crop contents written into the SAME tensors; the replay's loss
    equals an eager step of a copy of the model on those tables"""
    from video_classification_amd.slowfast import resnet50_2d_engine
    from video_classification_amd.train import TrainStep
    g = torch.Generator().manual_seed(9)
    n, t, s, f = 4, 4, 64, 24
    pad = s // 10
    arena = torch.randint(0, 256, (f, s, s, 21), generator=g, dtype=torch.uint8).to(DEV)
    index = torch.randint(0, f, (n, t), generator=g, dtype=torch.int32).to(DEV)
    crop = torch.randint(0, 2 * pad + 1, (n, 2), generator=g, dtype=torch.int32).to(DEV)
    lut = normalize_lut().to(DEV)
    labels = torch.tensor([0, 3, 5, 1], device=DEV)
    m = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    step = TrainStep(m.engine, lr=1e-3, use_graph=True)
    x = PoolClip(arena, index, 0, 5, crop, pad, lut, FILL)
    step(x, None, labels)                      # eager
    step(x, None, labels)                      # captured + replayed
    old_loss = float(step(x, None, labels))    # replay
    index.copy_(torch.tensor([[3, 3, -1, 0], [f, 5, 23, 22], [1, 2, 4, 8], [23, 0, 3, 3]], dtype=torch.int32))
    crop.copy_(torch.tensor([[0, 2 * pad], [2 * pad, 0], [3, 7], [2 * pad, 2 * pad]], dtype=torch.int32))
    twin = resnet50_2d_engine(7, t, s, dtype=torch.bfloat16, device=DEV, depth=18)
    twin.load_state_dict(m.state_dict(), strict=True)
    eager = TrainStep(twin.engine, lr=1e-3, use_graph=False)
    want = float(eager(PoolClip(arena, index.clone(), 0, 5, crop.clone(), pad, lut, FILL), None, labels))
    got = float(step(x, None, labels))         # replay of the captured graph
    assert step._cache and any(e["graph"] is not None for e in step._cache.values())
    assert got == pytest.approx(want, rel=1e-6, abs=1e-6) and got != old_loss


def _trainer(name, on):
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import SyntheticChalearn, Trainer
    cfg = get_cfg()
    cfg.CHALEARN.BATCH_SIZE = 4
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = "CropLHand"
    cfg.MODEL.DTYPE = "bf16"
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.RESIDENT_TRAIN = True
    cfg.MODEL.RESIDENT_GB = 40 * 64 * 64 * 21 / 2 ** 30           # 40 slots: 24 resident + the spill region of 16
    cfg.MODEL.POOL_STEM = on
    cfg.MODEL.LR = 1e-3
    cfg.NUM_CPU = 0
    tr = SyntheticChalearn(cfg, "train", num_videos=8, seed=1, as_uint8=True, frames_per_video=(3, 9))
    te = SyntheticChalearn(cfg, "test", num_videos=3, seed=2, pooled=True, frames_per_video=(4, 12))
    torch.manual_seed(0)
    return Trainer(cfg, train_set=tr, test_set=te, device=DEV)


@pytest.mark.parametrize("name", ["res2d", "res3d", "slowfast"])
def test_trainer_pool_stem_on_and_off(name):
    ts = [_trainer(name, on) for on in (False, True)]
    # the pooled run_eval (no filter gradient): identical scores
    ps = [t.run_eval()["ps"] for t in ts]
    assert ps[0].size > 0 and (ps[0] == ps[1]).all()
    assert not ts[0].frame_pool.live and not ts[1].frame_pool.live
    first, losses, seen = [], [[], []], [[], []]
    for k, t in enumerate(ts):
        t.model.train()
        for i, batch in enumerate(t.resident.epoch(0)):          # two steps
            x, y = t.mm.prepare_data(batch)
            seen[k].append(x)
            if i == 0:                                           # the first step's forward, loss and gradients, as
                logits = t.model(x)                              # test_gpu_u8_stem.py takes them: through autograd (the fused
                loss = torch.nn.functional.cross_entropy(logits.float(), y)   # step adds its loss with atomics)
                loss.backward()
                torch.cuda.synchronize()
                eng = t.model.engine
                stems = [eng._layers[st.conv_key] for st in eng.wiring.stems]
                first.append((logits.detach().clone(), loss.detach().clone(),
                              [eng._gslice(L.w_off, L.w_numel).clone() for L in stems], eng.G.clone()))
            if isinstance(x, (torch.Tensor, PoolClip)):
                losses[k].append(float(t.step(x, None, y)))
            else:
                losses[k].append(float(t.step(x[0], x[1], y, slow_t_index=t.model.slow_t_index)))
        torch.cuda.synchronize()
    assert len(losses[0]) == len(losses[1]) == 2 and ts[0].resident.spilled_clips == ts[1].resident.spilled_clips > 0
    assert all(torch.is_tensor(x) or torch.is_tensor(x[0]) for x in seen[0])
    assert all(isinstance(x, PoolClip) or all(isinstance(v, PoolClip) for v in x) for x in seen[1])
    print(f"{name}: first loss off {float(first[0][1])!r} on {float(first[1][1])!r}; fused losses off {losses[0]} on {losses[1]}")
    # the first step: logits and loss bit-equal
    assert torch.isfinite(first[0][0]).all() and float(first[0][0].float().abs().max()) > 0
    assert torch.equal(first[0][0], first[1][0]) and torch.equal(first[0][1], first[1][1])
    assert losses[0][0] == pytest.approx(losses[1][0], rel=1e-5), losses   # (the fused loss adds its batch with atomics)
    # the first step's gradients, to the tolerance test_gpu_u8_stem.py holds its U8_STEM on / off gradients to -- here also on each
    # STEM's filter gradient alone, relative to that stem's own largest element: the one gradient the pooled kernels compute
    for p, (g_off, g_on) in enumerate(zip(first[0][2], first[1][2])):
        print(f"{name}: stem {p} filter gradient rel_err {rel_err(g_on, g_off):.3e} cosine {cosine(g_on, g_off):.8f}")
        assert torch.isfinite(g_on).all() and float(g_off.abs().max()) > 0
        assert rel_err(g_on, g_off) < 2e-2 and cosine(g_on, g_off) > 0.9999
    assert rel_err(first[1][3], first[0][3]) < 2e-2 and cosine(first[1][3], first[0][3]) > 0.9999
    # after two steps the weights -- the parameters Adam updates; the BatchNorm running statistics beside them in the state dict
    # are not weights -- agree to 2e-2 of the largest value, the number test_gpu_u8_stem.py holds its U8_STEM on / off comparison
    # to.  Adam's first update is lr * sign(g), so an element whose gradient is at rounding level (the filter gradients add split
    # sums with fp32 atomics) moves by a full lr either way, as it does between two runs of either route: what this bound can
    # see is a step that went astray, not a wrong filter gradient, and the cosine of the weight vectors counts those sign flips
    # and not the kernels.  The gradient checks above are the ones with teeth; the cosine is printed, not asserted.
    w = [torch.cat([v.float().flatten() for k_, v in t.model.state_dict().items()
                    if not k_.endswith(("running_mean", "running_var", "num_batches_tracked"))]) for t in ts]
    print(f"{name}: weights rel_err {rel_err(w[1], w[0]):.3e} cosine {cosine(w[1], w[0]):.8f}")
    assert w[0].numel() > 1000 and torch.isfinite(w[1]).all() and rel_err(w[1], w[0]) < 2e-2
    assert ts[0].resident.bytes_uploaded == ts[1].resident.bytes_uploaded
    assert ts[0].resident.pool.live == ts[1].resident.pool.live
