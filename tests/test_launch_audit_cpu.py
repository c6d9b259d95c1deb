"""The launch audit's own pins, without a GPU: the float64 restatement (tests/ref64.py) against torch's float64 conv3d and
its autograd, the tolerance policy against rounded references and against the mutations a subtly wrong kernel makes, and
the recorder -> replay harness (tests/launch_audit.py) end to end on the CPU engine with EmuBackend playing the kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

import launch_audit as la
import ref64
from emu_backend import EmuBackend
from emu_stem2d import EmuStem2dBackend
from video_classification_amd import plan
from video_classification_amd._lib import stem_kp

D = torch.float64


def _cl(x):                       # (N,C,T,H,W) -> (N,T,H,W,C)
    return x.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("k,s,p", [((3, 3, 3), (1, 2, 2), (1, 1, 1)), ((1, 3, 3), (1, 1, 1), (0, 1, 1)),
                                   ((3, 1, 1), (1, 1, 1), (1, 0, 0)), ((1, 1, 1), (1, 2, 2), (0, 0, 0))])
def test_ref64_conv_dgrad_wgrad_match_conv3d_autograd(k, s, p):
    torch.manual_seed(0)
    g = plan.ConvGeom(8, 12, k, s, p)
    dims = (5, 9, 7)
    x = torch.randn(2, 8, *dims, dtype=D, requires_grad=True)
    w = torch.randn(12, 8, *k, dtype=D, requires_grad=True)
    y = F.conv3d(x, w, None, s, p)
    dy = torch.randn_like(y)
    y.backward(dy)
    W = w.detach().permute(0, 2, 3, 4, 1).reshape(12, g.wtaps, 8)          # [co][widx][ci]
    fp = plan.fwd_pass(g, dims)
    acc, a = ref64.conv(_cl(x.detach()), W, fp.rows, fp.gs, fp.taps)
    assert torch.allclose(acc, _cl(y.detach()), rtol=1e-12, atol=1e-12)
    assert (a >= acc.abs() - 1e-12).all()
    # data gradient: one pass per parity class, filter with (co, ci) swapped, scattered at r*os + oo
    Wt = W.permute(2, 1, 0).contiguous()
    dx = torch.zeros(2, *dims, 8, dtype=D)
    passes, _ = plan.dgrad_passes(g, dims)
    for ps in passes:
        v, _ = ref64.conv(_cl(dy), Wt, ps.rows, ps.gs, ps.taps)
        sl = ref64.region(ps.rows, ps.os, ps.oo)
        dx[:, sl[0], sl[1], sl[2]] += v
    assert torch.allclose(dx, _cl(x.grad), rtol=1e-12, atol=1e-12)
    dw, _ = ref64.wgrad(_cl(x.detach()), _cl(dy), g.s, plan.wgrad_taps(g), g.wtaps)
    assert torch.allclose(dw, w.grad.permute(0, 2, 3, 4, 1).reshape(12, g.wtaps, 8), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kt,t_index", [(1, [0, 3, 5]), (5, None), (3, [1, 2, 4, 6])])
def test_ref64_stem_matches_conv3d_with_frame_index(kt, t_index):
    torch.manual_seed(1)
    cin, cout = 3, 8
    src = torch.randn(2, cin, 7, 19, 18, dtype=D)
    ti = None if t_index is None else torch.tensor(t_index, dtype=torch.int32)
    kp = stem_kp(cin, kt)
    w = torch.randn(cout, kp, dtype=D)
    wt = ref64.stem_w(w.reshape(-1), cout, cin, kt, kp)                    # (cout, kt*49, cin)
    w5 = wt.view(cout, kt, 7, 7, cin).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    xs = src if ti is None else src.index_select(2, ti.long())
    y = F.conv3d(xs, w5, None, (1, 2, 2), (kt // 2, 3, 3))
    X = ref64.stem_x(src, ti, D)
    acc, _ = ref64.conv(X, wt, (X.shape[1], y.shape[3], y.shape[4]), (1, 2, 2), ref64.stem_taps(kt))
    assert torch.allclose(acc, _cl(y.detach()), rtol=1e-12, atol=1e-12)
    dy = torch.randn_like(y)
    y.backward(dy)
    g, _ = ref64.wgrad(X, _cl(dy), (1, 2, 2), ref64.stem_taps(kt), kt * 49)
    lay = ref64.stem_w_layout(g, cout, cin, kt)
    want = F.pad(w5.grad.permute(0, 2, 1, 3, 4), (0, 1)).reshape(cout, kt * cin * 56)
    assert torch.allclose(lay, want, rtol=1e-12, atol=1e-12)


def test_ref64_stem2d_matches_conv2d_over_stacked_frames():
    torch.manual_seed(2)
    n, c, t, h, w, cout = 2, 5, 3, 17, 16, 8
    src = torch.randn(n, c, t, h, w, dtype=D)
    kp = stem_kp(c, t)
    wl = torch.randn(cout, kp, dtype=D)
    W = ref64.stem_w(wl.reshape(-1), cout, c, t, kp).view(cout, t, 49, c).permute(0, 2, 1, 3).reshape(cout, 49, t * c)
    w2 = W.view(cout, 7, 7, t * c).permute(0, 3, 1, 2)
    x2 = src.permute(0, 2, 1, 3, 4).reshape(n, t * c, h, w)                # channel t*C + c
    y = F.conv2d(x2, w2, None, 2, 3)
    taps = [(0, kh - 3, kw - 3, kh * 7 + kw) for kh in range(7) for kw in range(7)]
    acc, _ = ref64.conv(ref64.stem2d_x(src, D), W, (1, y.shape[2], y.shape[3]), (1, 2, 2), taps)
    assert torch.allclose(acc[:, 0], y.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_ref64_stem_tail_matches_torch_maxpool_and_its_gradient():
    torch.manual_seed(3)
    a = torch.randn(2, 3, 11, 10, 4, dtype=D, requires_grad=True)
    out, arg = ref64.maxpool_fwd(a.detach(), 3, 2, 1)
    t = F.max_pool3d(a.permute(0, 4, 1, 2, 3), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    assert torch.equal(out, t.detach().permute(0, 2, 3, 4, 1))
    g = torch.randn_like(t)
    t.backward(g)
    da = ref64.maxpool_bwd(_cl(g), arg, 11, 10, 3, 2, 1)
    assert torch.allclose(da, a.grad, atol=1e-12)


def test_ref64_bn_kinds_match_emu_backend():
    """the BatchNorm restatements of the audit agree with EmuBackend's (the contract's torch statement)"""
    torch.manual_seed(4)
    be = EmuBackend()
    from helpers import empty_fmap
    y = empty_fmap(2, 16, 3, 5, 6)
    y.buf.normal_()
    da = y.like(torch.randn(y.pixels * 16))
    mean, invstd = torch.randn(16), torch.rand(16) + 0.5
    scale, shift = torch.randn(16), torch.randn(16)
    parts = torch.zeros(16 * 2)
    be.bn_bwd_reduce(da, y, None, mean, invstd, scale, shift, True, None, parts, 1)[0](0)
    outs = la._ref_bn_bwd_reduce(be, dict(da=da, y=y, mask_src=None, mean=mean, invstd=invstd, scale=scale, shift=shift,
                                          relu=True, dz_out=None, partials=parts, relu_bits=None), 1)
    v = ref64.compare("p", parts.view(1, 16, 2).double().sum(0), outs[0].ref, outs[0].a, outs[0].k, torch.float32, "sum_f32")
    assert v.ok, v
    st = torch.zeros(32)
    be.bn_stats(y, st, 1)[0](0)
    o = la._ref_bn_stats(be, dict(y=y, partials=st, max_parts=1), 1)[0]
    assert ref64.compare("s", st.view(16, 2), o.ref, o.a, o.k, torch.float32, "sum_f32").ok


# ----------------------------------------------------------------------------- the tolerance policy and its mutations
def _conv_case(n=2, t=3, h=20, w=20, cin=32, cout=16, k=(3, 3, 3), seed=5):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, t, h, w, cin, generator=g, dtype=D).to(torch.bfloat16).to(D)
    geo = plan.ConvGeom(cin, cout, k, (1, 1, 1), tuple(kk // 2 for kk in k))
    W = (torch.randn(cout, geo.wtaps, cin, generator=g, dtype=D) / math.sqrt(cin * geo.wtaps)).to(torch.bfloat16).to(D)
    fp = plan.fwd_pass(geo, (t, h, w))
    return X, W, fp, cin * geo.wtaps


def _verdict(y, r, a, k, dtype=torch.bfloat16, kind="map_bf16"):
    return ref64.compare("m", y, r, a, k, dtype, kind)


def test_tolerance_accepts_the_rounded_reference():
    X, W, fp, K = _conv_case()
    r, a = ref64.conv(X, W, fp.rows, fp.gs, fp.taps)
    assert _verdict(ref64.rounded(r, torch.bfloat16), r, a, K).ok
    assert _verdict(ref64.rounded(r, torch.float32), r, a, K, torch.float32, "map_f32").ok
    fp32 = ref64.conv(X.float(), W.float(), fp.rows, fp.gs, fp.taps)[0]      # an fp32-accumulated GEMM passes too
    assert _verdict(fp32.to(torch.bfloat16), r, a, K).ok


def test_tolerance_rejects_a_dropped_input_channel_of_one_tap():
    X, W, fp, K = _conv_case()
    r, a = ref64.conv(X, W, fp.rows, fp.gs, fp.taps)
    Wm = W.clone()
    Wm[:, fp.taps[4][3], 7] = 0
    y = ref64.conv(X, Wm, fp.rows, fp.gs, fp.taps)[0]
    assert not _verdict(ref64.rounded(y, torch.bfloat16), r, a, K).ok


def test_tolerance_rejects_a_zeroed_or_shifted_256_row_tile():
    X, W, fp, K = _conv_case()
    r, a = ref64.conv(X, W, fp.rows, fp.gs, fp.taps)
    flat = ref64.rounded(r, torch.bfloat16).reshape(-1, r.shape[-1])
    z = flat.clone()
    z[512:768] = 0
    assert not _verdict(z, r, a, K).ok
    s = flat.clone()
    s[512:768] = flat[513:769]
    assert not _verdict(s, r, a, K).ok


def test_tolerance_rejects_a_border_read_as_nonzero():
    X, W, fp, K = _conv_case()
    r, a = ref64.conv(X, W, fp.rows, fp.gs, fp.taps)
    Xp = F.pad(X, (0, 0, 1, 1, 1, 1, 1, 1), value=0.0)
    Xp[:, :, 0] = 0.25                                          # the row above h = 0 reads 0.25 instead of padding
    taps = [(dt + 1, dh + 1, dw + 1, wi) for dt, dh, dw, wi in fp.taps]
    y = ref64.conv(Xp, W, fp.rows, fp.gs, taps)[0]
    assert not _verdict(ref64.rounded(y, torch.bfloat16), r, a, K).ok


def test_tolerance_rejects_c_off_off_by_one():
    g = torch.Generator().manual_seed(6)
    wide = torch.randn(2, 3, 8, 8, 40, generator=g, dtype=D).to(torch.bfloat16).to(D)
    W = (torch.randn(16, 1, 32, generator=g, dtype=D) / math.sqrt(32)).to(torch.bfloat16).to(D)
    taps = [(0, 0, 0, 0)]
    r, a = ref64.conv(wide[..., 4:36], W, (3, 8, 8), (1, 1, 1), taps)
    y = ref64.conv(wide[..., 5:37], W, (3, 8, 8), (1, 1, 1), taps)[0]
    assert not _verdict(ref64.rounded(y, torch.bfloat16), r, a, 32).ok


def test_tolerance_rejects_a_missing_partial_row_of_the_stats():
    X, W, fp, K = _conv_case(n=4, h=32, w=32)
    acc, a = ref64.conv(X, W, fp.rows, fp.gs, fp.taps)
    flat, fa = acc.reshape(-1, acc.shape[-1]), a.reshape(-1, acc.shape[-1])
    rows = [flat[i:i + 256] for i in range(0, flat.shape[0], 256)]
    st = torch.stack([flat.sum(0), (flat * flat).sum(0)], -1)
    sa = torch.stack([fa.sum(0), (2 * flat.abs() * fa).sum(0)], -1)
    k = la._klen(flat.shape[0], K)
    part = torch.stack([torch.stack([b.sum(0), (b * b).sum(0)], -1) for b in rows]).float()
    assert ref64.compare("st", part.double().sum(0), st, sa, k, torch.float32, "sum_f32").ok
    assert not ref64.compare("st", part[1:].double().sum(0), st, sa, k, torch.float32, "sum_f32").ok


def test_tolerance_rejects_a_missing_64_pixel_k_tile_of_a_long_filter_gradient():
    """dW over 2^21 pixels (the stems' and res2's K is millions): one 64-pixel K-tile missing moves dW by ~sqrt(64/K)
    relative -- far inside the element-wise bound, so the aggregate bound must be the one that catches it"""
    g = torch.Generator().manual_seed(7)
    P, cin, cout = 1 << 21, 8, 8
    X = torch.randn(P, cin, generator=g, dtype=D).to(torch.bfloat16).to(D)
    dY = torch.randn(P, cout, generator=g, dtype=D).to(torch.bfloat16).to(D)
    r, a = dY.t() @ X, dY.abs().t() @ X.abs()
    good = (dY.t().float() @ X.float()).double()
    assert ref64.compare("dw", good, r, a, P, torch.float32, "sum_f32").ok
    miss = good - (dY[4096:4160].t() @ X[4096:4160]).float().double()
    v = ref64.compare("dw", miss, r, a, P, torch.float32, "sum_f32")
    assert v.worst <= 1.0 and not v.ok, v


# ----------------------------------------------------------------------------- the harness end to end on the CPU engine
def _mini_geometries():
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast, pack_pathway_index, resnet50_2d_engine

    def sf(be, dev):
        spec = arch.canonical_spec(7, depth=18, head_pool_kernels=((2, 2, 2), (8, 2, 2)))
        m = SlowFast(spec, dtype=torch.float32, device=dev, backend=be, seed=0)
        x = torch.randn(2, 3, 8, 64, 64)
        return m, x, x, pack_pathway_index(8, 4, dev)

    def r2d(be, dev):
        m = resnet50_2d_engine(7, clip_len=2, crop=64, dtype=torch.float32, device=dev, backend=be, seed=0, depth=18)
        return m, m.engine.input_view(torch.randn(2, 10, 64, 64)), None, None
    return {"sf": sf, "r2d": r2d}


def test_recorder_replay_end_to_end_on_the_cpu_engine():
    be = EmuStem2dBackend()
    rec = la.record_plans(be, "cpu", _mini_geometries())
    sigs = list(rec.calls)
    kinds = {s[0] for s in sigs}
    assert {"conv_igemm", "conv_wgrad", "stem_conv_fwd", "stem_conv_wgrad", "stem2d_fwd", "stem2d_wgrad",
            "bn_bwd_finalize"} <= kinds, kinds
    assert all(tags <= {"sf", "r2d"} for tags in rec.calls.values())
    bad = []
    for i, s in enumerate(sigs):
        r = la.replay(s, be, "cpu", seed=i)
        if not r.ok:
            bad.append((la.describe(s), r.verdicts, r.untouched_bad))
    assert not bad, bad[:3]


def test_replay_flags_a_write_outside_the_region_and_an_unknown_method():
    class Sloppy(EmuBackend):
        def bn_stats(self, y, partials, max_parts):
            run, n = super().bn_stats(y, partials, max_parts)

            def r(stream):
                run(stream)
                y.buf[-1] = 7.0          # touches the input map
            return r, n
    from helpers import empty_fmap
    rec = la.Recorder(Sloppy())
    y = empty_fmap(1, 8, 1, 4, 4)
    rec.bn_stats(y, torch.zeros(4 * 16), 4)
    (sig,) = rec.calls
    assert not la.replay(sig, Sloppy(), "cpu").ok
    assert la.replay(sig, EmuBackend(), "cpu").ok
    with pytest.raises(NotImplementedError):
        la.replay(("bn_tail_fwd",) + sig[1:], EmuBackend(), "cpu")
