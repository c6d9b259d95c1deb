"""The BatchNorm / max-pool / block-tail audit's own pins, without a GPU (tests/bn_ref64.py): the float64 restatements against
torch's float64 operators and their autograd; EmuBackend, the honest fp32 / bf16 implementation, inside the bound at EVERY case
the GPU test runs, with the share of ambiguous ReLU signs under its cap at every table entry; and the mutations a subtly wrong
kernel makes, each outside the bound in at least one case of the same tables."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref64 as B
import ref64
from emu_backend import EmuBackend
from video_classification_amd._lib import FMap

D = torch.float64
E32, M32 = B.f32(B.EPS), B.f32(B.MOMENTUM)      # the float32 values the C ABI carries


def close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


class Backend(EmuBackend):
    """kind None: EmuBackend as it stands, plus the [cout][4] coefficient scratch of sfk_bn_tail_bwd, which the emulation does
    not keep (the kernel leaves (A, B, C, 0) there and the GPU test reads it).  Any other kind: ONE corruption, the way a wrong
    kernel would make it; everything else stays honest."""

    def __init__(self, kind=None):
        self.kind = kind

    # ------------------------------------------------------------------ sfk_bn_apply
    def bn_apply(self, y, scale, shift, res, res_scale, res_shift, relu, out, relu_bits=None, out_sums=None, max_parts=0):
        k, V, c, px = self.kind, B.vec_of(y.dtype), y.c, y.pixels
        if k == "res_ld" and res is not None and y.ld >= res.c_off + c and res.buf.numel() >= px * y.ld:
            res = FMap(res.buf, res.n, res.t, res.h, res.w, c, y.ld, res.c_off)          # the residual read with y's ld
        if k == "swap_res" and res_scale is not None:
            res_scale, res_shift = res_shift, res_scale
        inner = super().bn_apply(y, scale, shift, res, res_scale, res_shift, relu, out, relu_bits, out_sums, max_parts)
        run0, nparts = inner if out_sums is not None else (inner, 0)

        def rows(m):
            return m.buf[: px * m.ld].view(px, m.ld)[:, m.c_off:m.c_off + c]

        def run(stream):
            before = rows(out).clone()
            pre = (y.view5().float() * scale[:c] + shift[:c]).reshape(px, c)          # fp32, before any rounding
            if k == "relu_first" and relu and res is not None:                        # ReLU, then the residual
                r = res.view5().float()
                if res_scale is not None:
                    r = r * res_scale[:c] + res_shift[:c]
                v = pre.clamp_min(0) + r.reshape(px, c)
                if relu_bits is not None:
                    relu_bits[: px * (c // V)] = ref64.relu_bits_pack(v > 0, V)
                rows(out).copy_(v.to(out.dtype))
                return
            run0(stream)
            if k == "skip_group":                                                     # the last channel group is never written
                rows(out)[:, -V:] = before[:, -V:]
            if k == "skip_rows":                                                      # the rows of the last partial span
                rem = px % (B.SPAN_U * B.rows_b(c, y.dtype))
                if rem:
                    rows(out)[px - rem:] = before[px - rem:]
            if k == "bit_rev" and relu_bits is not None:                              # bit i = channel V - 1 - i
                m = ref64.relu_bits_unpack(relu_bits, px, c, V).reshape(px, c // V, V).flip(-1).reshape(px, c)
                relu_bits[: px * (c // V)] = ref64.relu_bits_pack(m, V)
            if k == "sums_pre" and out_sums is not None:                              # summed before the rounding to the map's dtype
                out_sums[: 2 * c].view(c, 2)[:, 0] = pre.clamp_min(0).sum(0)
            if k == "chunk_off" and out_sums is not None and c > 256 * V:             # second chunk's columns at the first's offset
                row = out_sums[: 2 * c].view(c, 2)
                tail = row[256 * V:].clone()
                row[256 * V:] = B.SENT
                row[: tail.shape[0]] = tail
        return (run, nparts) if out_sums is not None else run

    # ------------------------------------------------------------------ sfk_bn_bwd_apply
    def bn_bwd_apply(self, da, y, mask_src, mean, invstd, scale, shift, relu, coef, dy):
        k, c = self.kind, y.c
        if k == "swap_c12":
            coef = coef[: c * 3].view(c, 3)[:, [0, 2, 1]].reshape(-1)
        if k == "mask_y" and relu and mask_src is None:                               # y > 0 instead of y * scale + shift > 0
            mask_src, relu = y, False
        if k == "no_invstd":
            invstd = torch.ones_like(invstd)
        return super().bn_bwd_apply(da, y, mask_src, mean, invstd, scale, shift, relu, coef, dy)

    # ------------------------------------------------------------------ sfk_bn_finalize
    def bn_finalize(self, partials, nparts, c, count, gamma, beta, eps, momentum, rm, rv, nbt, mean, invstd, scale, shift,
                    workspace=None):
        k = self.kind
        if k not in ("unb_invstd", "swap_mom", "biased_rv"):
            return super().bn_finalize(partials, nparts, c, count, gamma, beta, eps, momentum, rm, rv, nbt, mean, invstd, scale,
                                       shift, workspace)

        def run(stream):
            pt = partials[: nparts * c * 2].view(nparts, c, 2).double().sum(0)
            mu = pt[:, 0] / count
            var = (pt[:, 1] / count - mu * mu).clamp_min(0)
            unb = var * count / (count - 1) if count > 1 else var
            is_ = (1.0 / torch.sqrt((unb if k == "unb_invstd" else var) + eps)).float()
            mean[:c], invstd[:c] = mu.float(), is_
            scale[:c] = gamma[:c] * is_
            shift[:c] = beta[:c] - mu.float() * scale[:c]
            if rm is not None:
                keep, new = (momentum, 1 - momentum) if k == "swap_mom" else (1 - momentum, momentum)
                rm[:c] = keep * rm[:c] + new * mu.float()
                rv[:c] = keep * rv[:c] + new * (var if k == "biased_rv" else unb).float()
            if nbt is not None:
                nbt.add_(1)
        return run

    # ------------------------------------------------------------------ max-pool
    def maxpool_fwd(self, x, y, argmax, k, s, p):
        kind = self.kind
        run0 = super().maxpool_fwd(x, y, argmax, k, s, p)

        def run(stream):
            run0(stream)
            if kind == "last_tie":                                                    # >= : the LAST maximum of the window
                X = x.view5().double()
                best = torch.full(y.view5().shape, -float("inf"), dtype=D)
                arg = torch.zeros(y.view5().shape, dtype=torch.uint8)
                for kh in range(k):
                    for kw in range(k):
                        hi, wi = torch.arange(y.h) * s - p + kh, torch.arange(y.w) * s - p + kw
                        ok = ((hi >= 0) & (hi < x.h)).view(1, 1, -1, 1, 1) & ((wi >= 0) & (wi < x.w)).view(1, 1, 1, -1, 1)
                        v = ref64.gather(X, (x.t, y.h, y.w), (1, s, s), (0, kh - p, kw - p))
                        take = ok & (v >= best)
                        best = torch.where(take, v, best)
                        arg = torch.where(take, torch.full_like(arg, kh * k + kw), arg)
                y.view5().copy_(best.to(y.dtype))
                argmax[: arg.numel()].view_as(arg).copy_(arg)
            if kind == "pad_zero":                                                    # padding taps enter the maximum as zeros
                h0, w0 = torch.arange(y.h) * s - p, torch.arange(y.w) * s - p
                padded = ((h0 < 0) | (h0 + k > x.h)).view(1, 1, -1, 1, 1) | ((w0 < 0) | (w0 + k > x.w)).view(1, 1, 1, -1, 1)
                v = y.view5().float()
                y.view5().copy_(torch.where(padded, v.clamp_min(0), v).to(y.dtype))
        return run

    def maxpool_bwd(self, dy, argmax, dx, k, s, p):
        if self.kind != "drop_second":
            return super().maxpool_bwd(dy, argmax, dx, k, s, p)

        def run(stream):                                                              # only the first window that routes here counts
            G = dy.view5().float()
            arg = argmax[: G.numel()].view(G.shape)
            out = torch.zeros(dx.n, dx.t, dx.h, dx.w, dx.c)
            hit = torch.zeros(out.shape, dtype=torch.bool)
            for ho in range(dy.h):
                for wo in range(dy.w):
                    for kh in range(k):
                        for kw in range(k):
                            hi, wi = ho * s - p + kh, wo * s - p + kw
                            if 0 <= hi < dx.h and 0 <= wi < dx.w:
                                sel = arg[:, :, ho, wo] == kh * k + kw
                                out[:, :, hi, wi] += G[:, :, ho, wo] * (sel & ~hit[:, :, hi, wi])
                                hit[:, :, hi, wi] |= sel
            dx.view5().copy_(out.to(dx.dtype))
        return run

    # ------------------------------------------------------------------ the block tail
    def bn_tail_fwd(self, gram, a_sums, a_nparts, count, g, c, w, cout, gamma, beta, eps, momentum, rm, rv, nbt, mean, invstd,
                    scale, shift, t, wd=None):
        k = self.kind
        run0 = super().bn_tail_fwd(gram, a_sums, a_nparts, count, g, c, w, cout, gamma, beta, eps, momentum, rm, rv, nbt, mean,
                                   invstd, scale, shift, t, wd)

        def run(stream):
            rm0, rv0 = (rm.clone(), rv.clone()) if rm is not None else (None, None)
            run0(stream)
            W = w[: cout * c].view(cout, c)
            if k == "uncentred":              # var = E[y^2] - E[y]^2 from an fp32 T = W G, in fp32
                n = torch.tensor(float(count))
                T32 = W.float() @ gram[: c * c].view(c, c)
                mu = (W.float() @ g[:c]) / n
                var = ((T32 * W.float()).sum(1) / n - mu * mu).clamp_min(0)
                is_ = 1.0 / torch.sqrt(var + eps)
                invstd[:cout], scale[:cout] = is_, gamma[:cout] * is_
                shift[:cout] = beta[:cout] - mu * scale[:cout]
                if rm is not None:
                    rv[:cout] = (1 - momentum) * rv0[:cout] + momentum * var * (count / (count - 1.0))
                if wd is not None:
                    wd[: cout * c].copy_((scale[:cout, None] * W.float()).t().reshape(-1).to(wd.dtype))
            if k == "wd_no_T" and wd is not None:                                     # (A W) left as [cout][c]
                wd[: cout * c].copy_((scale[:cout, None] * W.float()).reshape(-1).to(wd.dtype))
        return run

    def bn_tail_bwd(self, r, dz_partials, nparts, g_in, count, t, c, w, cout, gamma, mean, invstd, dgamma, dbeta, dw, m, bias,
                    coef):
        k = self.kind

        def run(stream):          # EmuBackend.bn_tail_bwd line by line, with the corruption of `kind` and the coefficient scratch
            R = r[: cout * c].view(cout, c).double()
            s_ = dz_partials[: nparts * cout * 2].view(nparts, cout, 2)[:, :, 0].double().sum(0)
            g, n = g_in[:c].double(), float(count)
            W = w[: cout * c].view(cout, c).double()
            T = t[: cout * c].view(cout, c).double()
            is_, mu = invstd[:cout].double(), mean[:cout].double()
            sxh = is_ * ((W * R).sum(1) - mu * s_)
            dgamma[:cout].add_(sxh.float())
            dbeta[:cout].add_(s_.float())
            A = gamma[:cout].double() * is_
            c1, c2 = s_ / n, sxh / n
            Bc = -A * c2 * is_
            if k == "b_sign":
                Bc = -Bc
            Cc = A * ((0.0 if k == "c_no_mean" else c2 * is_ * mu) - c1)
            coef[: cout * 4].view(cout, 4).copy_(torch.stack([A, Bc, Cc, torch.zeros_like(A)], 1).float())
            cg = 0.0 if k == "dw_no_cg" else Cc[:, None] * g[None, :]
            dw[: cout * c].add_((A[:, None] * R + Bc[:, None] * T + cg).float().reshape(-1))
            rows = slice(0, 16) if k == "m_slab16" else slice(0, cout)
            m[: c * c].copy_((W[rows].t() @ (Bc[rows, None] * W[rows])).reshape(-1).to(m.dtype))
            bias[:c].copy_((Cc @ W).float())
        return run


def _accepts(vs):
    assert not B.failures(vs), B.failures(vs)[:4]


# ----------------------------------------------------------------------------- the restatements against torch float64
@pytest.mark.parametrize("res_mode,relu", [(0, False), (0, True), (1, True), (2, True), (2, False)])
def test_ref64_bn_matches_batch_norm_training_and_autograd(res_mode, relu):
    """finalize_ref -> apply_ref forward, bwd_finalize_ref -> bwd_apply_ref backward, against F.batch_norm(training=True) with
    its running-statistics update"""
    g0 = torch.Generator().manual_seed(0)
    n, c = 37, 6
    rn = lambda *s: torch.randn(*s, dtype=D, generator=g0)
    x = (rn(n, c) * 1.5 + 0.7).requires_grad_(True)
    gamma, beta = (rn(c) * 0.3 + 1).requires_grad_(True), rn(c).requires_grad_(True)
    rm, rv = rn(c), torch.rand(c, dtype=D, generator=g0) + 0.5
    res, rs, rb = (rn(n, c) if res_mode else None), (rn(c) if res_mode == 2 else None), (rn(c) if res_mode == 2 else None)
    trm, trv = rm.clone(), rv.clone()
    out = F.batch_norm(x, trm, trv, gamma, beta, True, M32, E32)
    if res_mode:
        out = out + (res * rs + rb if res_mode == 2 else res)
    if relu:
        out = out.relu()
    gout = rn(n, c)
    out.backward(gout)
    xd = x.detach()
    s1, s2 = xd.sum(0), (xd * xd).sum(0)
    ref = B.finalize_ref(s1, s1.abs(), s2, s2, n, gamma.detach(), beta.detach(), B.EPS, B.MOMENTUM, rm, rv)
    assert close(ref["rm"][0], trm) and close(ref["rv"][0], trv)
    assert close(ref["mean"][0], xd.mean(0)) and close(ref["var"][0], xd.var(0, unbiased=False))
    v, a, _ = B.apply_ref(xd, ref["scale"][0], ref["shift"][0], res, rs, rb)
    assert close(v.clamp_min(0) if relu else v, out.detach()) and (a >= v.abs() - 1e-12).all()
    mask = (v > 0) if relu else torch.ones_like(v, dtype=torch.bool)
    dz = gout * mask
    xh = (xd - ref["mean"][0]) * ref["invstd"][0]
    t1, t2 = dz.sum(0), (dz * xh).sum(0)
    zero = torch.zeros(c, dtype=D)
    bref = B.bwd_finalize_ref(t1, t1.abs(), t2, t2.abs(), n, gamma.detach(), ref["invstd"][0], zero, zero)
    assert close(bref["dgamma"][0], gamma.grad) and close(bref["dbeta"][0], beta.grad)
    coef = torch.stack([bref[f"coef{j}"][0] for j in range(3)], 1)
    dx, adx = B.bwd_apply_ref(gout, xd, mask, ref["mean"][0], ref["invstd"][0], coef)
    assert close(dx, x.grad) and (adx >= dx.abs() - 1e-12).all()


def test_ref64_unbiased_variance_guard_at_count_one():
    one = torch.ones(2, dtype=D)
    ref = B.finalize_ref(one * 3, one * 3, one * 9.5, one * 9.5, 1, one, one, B.EPS, B.MOMENTUM, one, one)
    assert close(ref["rv"][0], (1 - M32) * one + M32 * 0.5)


def test_ref64_eval_coeffs_match_batch_norm_eval():
    g0 = torch.Generator().manual_seed(1)
    n, c = 9, 65
    rn = lambda *s: torch.randn(*s, dtype=D, generator=g0)
    x, gamma, beta, rm, rv = rn(n, c), rn(c), rn(c), rn(c), torch.rand(c, dtype=D, generator=g0) + 0.5
    ref = B.eval_coeffs_ref(gamma, beta, rm, rv, B.EPS)
    assert close(x * ref["scale"][0] + ref["shift"][0], F.batch_norm(x, rm, rv, gamma, beta, False, M32, E32))


@pytest.mark.parametrize("case", [c for c in B.POOL_CASES if c["dtype"] == B.F32 and c["fill"] != "nan"], ids=B.pool_name)
def test_ref64_maxpool_matches_max_pool3d_indices_and_autograd(case):
    k, s, p, h, w = case["k"], case["s"], case["p"], case["h"], case["w"]
    g0 = torch.Generator().manual_seed(2)
    x5 = B.pool_input(case, g0)
    best, arg = ref64.maxpool_fwd(x5, k, s, p)
    tv, targ = B.torch_pool(x5, k, s, p)
    assert torch.equal(best, tv) and torch.equal(arg, targ)
    xt = x5.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    out = F.max_pool3d(xt, (1, k, k), (1, s, s), (0, p, p))
    gout = torch.randn(out.shape, dtype=D, generator=g0)
    out.backward(gout)
    assert close(ref64.maxpool_bwd(gout.permute(0, 2, 3, 4, 1), arg, h, w, k, s, p), xt.grad.permute(0, 2, 3, 4, 1))


@pytest.mark.parametrize("c,cout", [(8, 4), (24, 36)])
def test_ref64_tail_matches_conv_batchnorm3d_shortcut_relu_and_autograd(c, cout):
    """conv1x1 -> BatchNorm3d (training) -> + shortcut -> ReLU in torch float64 against tail_fwd_ref / tail_bwd_ref fed with
    G = a^T a, g = 1^T a, R = dz^T a, s = 1^T dz: the statistics, the running update, the output, and every gradient --
    da as dz wd^T + a m + bias, the two data-gradient passes the tail's operands are made for"""
    g0 = torch.Generator().manual_seed(3)
    px = 53
    rn = lambda *s: torch.randn(*s, dtype=D, generator=g0)
    a = (rn(px, c) + 0.5).clamp_min(0).requires_grad_(True)
    W = (rn(cout, c) * c ** -0.5).requires_grad_(True)
    bn = torch.nn.BatchNorm3d(cout, eps=E32, momentum=M32).double()
    rm, rv = rn(cout), torch.rand(cout, dtype=D, generator=g0) + 0.5
    with torch.no_grad():
        bn.weight.copy_(rn(cout) * 0.3 + 1)
        bn.bias.copy_(rn(cout))
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    shortcut, gout = rn(px, cout), rn(px, cout)
    y = F.conv3d(a.t().reshape(1, c, px, 1, 1), W.reshape(cout, c, 1, 1, 1))
    out = (bn(y).reshape(cout, px).t() + shortcut).relu()
    out.backward(gout)
    ad, Wd, gamma, beta = a.detach(), W.detach(), bn.weight.detach(), bn.bias.detach()
    ref = B.tail_fwd_ref(ad.t() @ ad, ad.sum(0), px, Wd, gamma, beta, B.EPS, B.MOMENTUM, rm, rv)
    yd = ad @ Wd.t()
    assert close(ref["mean"][0], yd.mean(0)) and close(ref["var"][0], yd.var(0, unbiased=False))
    assert close(ref["rm"][0], bn.running_mean) and close(ref["rv"][0], bn.running_var) and int(bn.num_batches_tracked) == 1
    assert close(ref["t"][0], Wd @ (ad.t() @ ad))
    pre = yd * ref["scale"][0] + ref["shift"][0] + shortcut
    assert close(pre.clamp_min(0), out.detach())
    dz = gout * (pre > 0)
    zc = torch.zeros(cout, dtype=D)
    s = dz.sum(0)
    b = B.tail_bwd_ref(dz.t() @ ad, s, s.abs(), ad.sum(0), px, ref["t"][0], Wd, gamma, ref["mean"][0], ref["invstd"][0], zc, zc,
                       torch.zeros(cout, c, dtype=D))
    assert close(b["dgamma"][0], bn.weight.grad) and close(b["dbeta"][0], bn.bias.grad) and close(b["dw"][0], W.grad)
    assert close(dz @ ref["wd"][0].t() + ad @ b["m"][0] + b["bias"][0], a.grad)
    for name in ("B", "C", "dw", "m", "bias"):
        assert (b[name][1] >= b[name][0].abs() - 1e-12).all(), name


# ----------------------------------------------------------------------------- honest fp32 / bf16 is inside the bound, everywhere
GROUP_IDS = [f"{B.tag_of(d)}-{cm}groups" for d, cm in B.APPLY_GROUPS]


def _relu_cases_state_their_ambiguity(case, vs):
    if case.get("relu") or case.get("mask") == 1:
        amb = [v for v in vs if v.name.startswith("ambiguous ReLU signs")]
        assert len(amb) == 1 and amb[0].ok, (B.case_name(case), amb)


@pytest.mark.parametrize("dtype,cm", B.APPLY_GROUPS, ids=GROUP_IDS)
def test_honest_bn_apply_is_inside_the_bound(dtype, cm):
    for case in B.group_of(B.APPLY_CASES + B.SUMS_CASES, dtype, cm):
        vs = B.check_apply(Backend(), "cpu", case)
        _accepts(vs)
        _relu_cases_state_their_ambiguity(case, vs)


@pytest.mark.parametrize("dtype,cm", B.APPLY_GROUPS, ids=GROUP_IDS)
def test_honest_bn_bwd_apply_is_inside_the_bound(dtype, cm):
    for case in B.group_of(B.BWD_APPLY_CASES, dtype, cm):
        vs = B.check_bwd_apply(Backend(), "cpu", case)
        _accepts(vs)
        _relu_cases_state_their_ambiguity(case, vs)


def test_the_case_tables_take_every_path_the_issue_names():
    for dtype in (B.BF16, B.F32):
        V = B.vec_of(dtype)
        assert [B.rows_b(cm * V, dtype) for cm in B.CMULS] == [256, 25, 1, 1]
        for cm in B.CMULS:
            rb = B.rows_b(cm * V, dtype)
            px = {c["px"] for c in B.group_of(B.APPLY_CASES, dtype, cm)}
            assert 1 in px and {(p % (B.SPAN_U * rb) + rb - 1) // rb for p in px if p > B.SPAN_U * rb} >= {1, 2, 3}
            assert rb <= 2 or any(1 < p < rb for p in px)
    assert any(c["alias"] for c in B.APPLY_CASES)
    assert {c["sums"] for c in B.SUMS_CASES} == {1, 3, 1024}
    assert {(c["c"], c["cout"]) for c in B.TAIL_CASES if not c["md"]} == set(B.TAIL_SHAPES)
    assert {c["a_np"] for c in B.TAIL_CASES} >= {1, 63, 65, 200} and sum(c["md"] for c in B.TAIL_CASES) == 1
    assert {c["nparts"] for c in B.FIN_CASES} == {1, 255, 257, 4097, 50176}
    assert B.CAP_PX == 4 * 65535 + 1030 and B.streamed_px(150) == 150 * 2 ** 20 // 128 + 37


@pytest.mark.parametrize("c", sorted({c["c"] for c in B.FIN_CASES}))
def test_honest_finalize_is_inside_the_bound(c):
    for case in (k for k in B.FIN_CASES if k["c"] == c):
        _accepts(B.check_finalize(Backend(), "cpu", case))


@pytest.mark.parametrize("c", B.EVAL_C)
def test_honest_eval_coeffs_are_inside_the_bound(c):
    _accepts(B.check_eval_coeffs(Backend(), "cpu", c))


def test_honest_maxpool_is_exact_and_inside_the_bound():
    for case in B.POOL_CASES:
        _accepts(B.check_pool(Backend(), "cpu", case))


@pytest.mark.parametrize("shape", B.TAIL_SHAPES, ids=[f"c{c}-cout{co}" for c, co in B.TAIL_SHAPES])
def test_honest_tail_is_inside_the_bound(shape):
    for case in (c for c in B.TAIL_CASES if (c["c"], c["cout"]) == shape):
        _accepts(B.check_tail(Backend(), "cpu", case))


def test_the_large_launch_checks_accept_the_honest_backend_at_a_small_size():
    """the grid-cap and streamed checks are sized for the GPU; their own code is run here on a few spans"""
    _accepts(B.check_grid_cap_apply(Backend(), "cpu", px=4 * 7 + 3, c=16))
    _accepts(B.check_grid_cap_bwd_apply(Backend(), "cpu", px=4 * 7 + 3, c=16))
    _accepts(B.check_streamed_bwd_apply(Backend(), "cpu", 1000, chunk=300))
    bad = Backend("skip_rows")
    assert B.failures(B.check_grid_cap_apply(bad, "cpu", px=4 * 7 + 3, c=16))


# ----------------------------------------------------------------------------- every mutation is outside the bound somewhere
MUTATIONS = {
    "res_ld": (B.APPLY_CASES, B.check_apply), "skip_group": (B.APPLY_CASES, B.check_apply),
    "skip_rows": (B.APPLY_CASES, B.check_apply), "relu_first": (B.APPLY_CASES, B.check_apply),
    "swap_res": (B.APPLY_CASES, B.check_apply), "bit_rev": (B.APPLY_CASES, B.check_apply),
    "sums_pre": (B.SUMS_CASES, B.check_apply), "chunk_off": (B.SUMS_CASES, B.check_apply),
    "swap_c12": (B.BWD_APPLY_CASES, B.check_bwd_apply), "mask_y": (B.BWD_APPLY_CASES, B.check_bwd_apply),
    "no_invstd": (B.BWD_APPLY_CASES, B.check_bwd_apply),
    "unb_invstd": (B.FIN_CASES, B.check_finalize), "swap_mom": (B.FIN_CASES, B.check_finalize),
    "biased_rv": (B.FIN_CASES, B.check_finalize),
    "last_tie": (B.POOL_CASES, B.check_pool), "pad_zero": (B.POOL_CASES, B.check_pool), "drop_second": (B.POOL_CASES, B.check_pool),
    "uncentred": (B.TAIL_CASES, B.check_tail), "b_sign": (B.TAIL_CASES, B.check_tail), "c_no_mean": (B.TAIL_CASES, B.check_tail),
    "dw_no_cg": (B.TAIL_CASES, B.check_tail), "wd_no_T": (B.TAIL_CASES, B.check_tail), "m_slab16": (B.TAIL_CASES, B.check_tail),
}


@pytest.mark.parametrize("kind", sorted(MUTATIONS))
def test_mutation_is_outside_the_bound(kind):
    cases, check = MUTATIONS[kind]
    rejected = 0
    for case in cases:
        if B.failures(check(Backend(kind), "cpu", case)):
            rejected += 1
            if rejected >= 2:
                break
    assert rejected >= 1, kind
