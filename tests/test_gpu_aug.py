"""sfk_color_jitter on an MI355X (include/sfk_aug.h) against tests/ref_jitter.py in float64: all 24 op orders on frames that
take the scalar tail (17x19) and the 16-byte path (32x32), three layouts, f32 and bf16, untouched memory, reproducibility,
skipped slots, a captured graph following new params, gesture_v2's prepare_data and one mini v2 Trainer epoch.

The bound is not a constant: E32 is the largest |ref_jitter in float32 - ref_jitter in float64| on the same inputs, in stored
units, and the kernel must stay within 4 * E32 of the float64 result on EVERY element (both sides are fp32 evaluations of
one formula that differ only in contraction and in the order of the mean's sum).  Measured (stored units): DESIGN.md section 9."""
import functools
import itertools
import math

import pytest
import torch

from ref_jitter import ref_jitter
from video_classification_amd._lib import HipBackend
from video_classification_amd.input_pipeline import draw_color_jitter, normalize_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(17, 19), (32, 32)]
# name -> (channels, c_off, bgr, mean, std, floats between two clips)
LAYOUTS = {"7ch": (7, 0, False, 0.0, 1.0, 0), "21ch_bgr_norm": (21, 0, True, 0.45, 0.225, 0), "strided_sn": (7, 2, False, 0.0, 1.0, 5)}
PERMS = list(itertools.permutations(range(4)))


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def case(h, w, layout):
    """(stored clip (24, 2, C, h, w) float32 on the host, params (24, 8)): bytes / 255 (normalised for the v1 layout) with gray
    rows, r == g rows, an all-0 row and an all-255 row planted in the three colour planes"""
    c, c_off, bgr, mean, std, _ = LAYOUTS[layout]
    g = torch.Generator().manual_seed(h * 100 + w)
    u = torch.randint(0, 256, (24, 2, c, h, w), generator=g, dtype=torch.uint8)
    rgb = u[:, :, c_off:c_off + 3]
    rgb[:, :, :, 0] = rgb[:, :, 0:1, 0].clone()                    # gray rows: r == g == b
    rgb[:, :, :, 5] = rgb[:, :, 1:2, 5].clone()
    rgb[:, :, 1, 2] = rgb[:, :, 0, 2].clone()                      # r == g (or b == g) ties
    rgb[:, :, 1, 7] = rgb[:, :, 2, 7].clone()
    rgb[:, :, :, 3] = 0
    rgb[:, :, :, 9] = 255
    x = normalize_lut(mean, std)[u.long()] if std != 1.0 else u.to(torch.float32).div(255)
    params = draw_color_jitter(24, 0.5, 0.3, 0.2, 0.5, g)
    params[:, :4] = torch.tensor(PERMS, dtype=torch.float32)
    return x, params


@functools.lru_cache(maxsize=None)
def refs(h, w, layout):
    """(float64 reference, E32) of case(h, w, layout), computed once"""
    x, params = case(h, w, layout)
    _, c_off, bgr, mean, std, _ = LAYOUTS[layout]
    r64 = ref_jitter(x.double(), params, c_off, bgr, mean, std)
    r32 = ref_jitter(x, params, c_off, bgr, mean, std)
    return r64, float((r32.double() - r64).abs().max())


def on_device(x, gap=0, dtype=torch.float32, guard=64):
    """x in a pattern-filled device buffer with `gap` elements between two clips and `guard` after the last: (view, buffer)"""
    n = x.shape[0]
    per = x[0].numel()
    buf = torch.arange(n * (per + gap) + guard, dtype=torch.float32).mul_(0.37).sub_(11).to(dtype).to(DEV)
    view = buf[:n * (per + gap)].view(n, per + gap)[:, :per].view(x.shape)
    view.copy_(x.to(dtype))
    return view, buf


def run_kernel(view, params, c_off, bgr, mean, std, be=None):
    be = be or HipBackend()
    n, t, _, h, w = view.shape
    ws = torch.full((be.color_jitter_workspace_bytes(n, t, h, w) // 4,), float("nan"), device=DEV)
    be.color_jitter(view, params.to(DEV), ws, c_off, bgr, mean, std)(stream())
    torch.cuda.synchronize()
    return view


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("h,w", SIZES)
def test_parity_with_float64_all_orders(h, w, layout):
    x, params = case(h, w, layout)
    _, c_off, bgr, mean, std, gap = LAYOUTS[layout]
    r64, e32 = refs(h, w, layout)
    view, _ = on_device(x, gap)
    assert (view.stride(0) != view[0].numel()) == (gap != 0)
    got = run_kernel(view, params, c_off, bgr, mean, std).cpu()
    err = float((got.double() - r64).abs().max())
    print(f"jitter parity {h}x{w} {layout}: E32 {e32:.3e} kernel {err:.3e}")
    assert 0 < e32 < 1e-4 and torch.isfinite(got).all()
    assert err <= 4 * e32, (err, e32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("h,w", SIZES)
def test_memory_outside_the_three_planes_is_untouched(h, w, dtype):
    x, params = case(h, w, "strided_sn")
    _, c_off, bgr, mean, std, gap = LAYOUTS["strided_sn"]
    view, buf = on_device(x, gap, dtype)
    before = buf.clone()
    run_kernel(view, params, c_off, bgr, mean, std)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    changed = (buf.view(bits) != before.view(bits))
    assert changed.any()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    n = x.shape[0]
    iv = inside[:n * (x[0].numel() + gap)].view(n, -1)[:, :x[0].numel()].view(x.shape)
    iv[:, :, c_off:c_off + 3] = True
    assert not (changed & ~inside).any()          # the other channels, the gaps between clips, the guard band


@pytest.mark.parametrize("layout", ["7ch", "21ch_bgr_norm"])
@pytest.mark.parametrize("h,w", SIZES)
def test_bf16_equals_f32_kernel_rounded(h, w, layout):
    x, params = case(h, w, layout)
    _, c_off, bgr, mean, std, _ = LAYOUTS[layout]
    xb = x.to(torch.bfloat16)
    vb, _ = on_device(xb, 0, torch.bfloat16)
    vf, _ = on_device(xb.float(), 0, torch.float32)
    gb = run_kernel(vb, params, c_off, bgr, mean, std)
    gf = run_kernel(vf, params, c_off, bgr, mean, std)
    assert gb.dtype == torch.bfloat16 and torch.equal(gb, gf.to(torch.bfloat16))
    assert not torch.equal(gb[:, :, c_off:c_off + 3].cpu(), xb[:, :, c_off:c_off + 3])


def test_two_runs_are_bit_equal():
    x, params = case(32, 32, "21ch_bgr_norm")
    _, c_off, bgr, mean, std, _ = LAYOUTS["21ch_bgr_norm"]
    a = run_kernel(on_device(x)[0], params, c_off, bgr, mean, std)
    b = run_kernel(on_device(x)[0], params, c_off, bgr, mean, std)
    assert torch.equal(a, b)


@pytest.mark.parametrize("h,w", SIZES)
def test_skipped_slots_and_clips_without_contrast(h, w):
    x, params = case(h, w, "7ch")
    p = params.clone()
    p[0::3, 1] = -1.0                                   # one slot skipped, whatever op it held
    p[1::3, :4] = torch.where(p[1::3, :4] == 1.0, torch.tensor(-1.0), p[1::3, :4])      # no contrast: pass 1 exits at once
    p[2, :4] = -1.0                                     # nothing at all: the clip comes back as it was
    p[5, :4] = 7.0
    r64 = ref_jitter(x.double(), p)
    e32 = float((ref_jitter(x, p).double() - r64).abs().max())
    got = run_kernel(on_device(x)[0], p, 0, False, 0.0, 1.0).cpu()
    err = float((got.double() - r64).abs().max())
    print(f"jitter skipped slots {h}x{w}: E32 {e32:.3e} kernel {err:.3e}")
    assert err <= 4 * e32, (err, e32)
    assert torch.equal(got[2], x[2]) and torch.equal(got[5], x[5])
    assert float((r64 - ref_jitter(x.double(), params)).abs().max()) > 1e-2       # leaving the ops out is a different result


def test_captured_graph_follows_new_params():
    x, params = case(32, 32, "7ch")
    be = HipBackend()
    view, _ = on_device(x)
    src = view.clone()
    pd = params.to(DEV)
    ws = torch.empty(be.color_jitter_workspace_bytes(24, 2, 32, 32) // 4, device=DEV)
    run = be.color_jitter(view, pd, ws)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    view.copy_(src)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(stream())
    for shift in (5, 11):
        p = params.roll(shift, 0).contiguous()
        pd.copy_(p)
        view.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        r64 = ref_jitter(x.double(), p)
        e32 = float((ref_jitter(x, p).double() - r64).abs().max())
        assert float((view.cpu().double() - r64).abs().max()) <= 4 * e32, shift


def _cfg(root="/nonexistent", jitter=False):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = str(root)
    cfg.CHALEARN.BATCH_SIZE = 2
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = "gesture-v2"
    cfg.MODEL.INPUT_SIZE = 64
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.COLOR_JITTER = jitter
    cfg.NUM_CPU = 0
    return cfg


def test_v2_prepare_data_on_the_device_against_the_emulated_jitter():
    from emu_aug import EmuAugBackend
    from video_classification_amd import gesture_v2 as v2
    g = torch.Generator().manual_seed(8)
    ub = {"frames_u8": torch.randint(0, 256, (2, 4, 120, 160, 7), generator=g, dtype=torch.uint8),
          "box": torch.tensor([[10, 4, 110, 117], [37, 0, 160, 90]], dtype=torch.int32),
          "crop": torch.tensor([[0, 9], [12, 4]], dtype=torch.int32), "label": torch.tensor([2, 6])}
    jit = draw_color_jitter(2, generator=g)
    mm = v2.ModelManager(_cfg(), DEV)
    (ps, pf), _ = mm.prepare_data(ub)
    plain = torch.cat([ps, pf], 1).permute(0, 2, 1, 3, 4).contiguous().cpu()        # (N, T, 7, S, S), unjittered
    (js, jf), _ = mm.prepare_data(dict(ub, jitter=jit))
    torch.cuda.synchronize()
    got = torch.cat([js, jf], 1).permute(0, 2, 1, 3, 4).cpu()
    emu = plain.clone()
    EmuAugBackend().color_jitter(emu, jit, None)(0)                                 # the emulated path's jitter step
    r64 = ref_jitter(plain.double(), jit)
    e32 = float((emu.double() - r64).abs().max())
    err = float((got.double() - r64).abs().max())
    print(f"jitter prepare_data: E32 {e32:.3e} kernel {err:.3e}")
    assert err <= 4 * e32, (err, e32)
    assert torch.equal(got[:, :, 3:], plain[:, :, 3:]) and not torch.equal(got[:, :, :3], plain[:, :, :3])


def test_mini_v2_trainer_epoch_with_color_jitter(tmp_path):
    from video_classification_amd import gesture_v2 as v2
    cfg = _cfg(tmp_path, jitter=True)
    cfg.MODEL.LR = 1e-2
    tr = v2.SyntheticGesture(cfg, "train", num_videos=5, seed=1, h=48, w=64, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    assert "jitter" in tr[0] and "jitter" not in te[0][0]
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device=DEV)
    loss, _ = t.train_epoch()
    assert t.step.steps == 3 and math.isfinite(loss)
    assert sorted(t.mm.color_jitter()._ws) == [(1, 4, 64, 64), (2, 4, 64, 64)]
