"""The head / loss / optimizer audit's own pins, without a GPU (tests/head_ref64.py): the float64 restatements against
torch's float64 operators and their autograd; an honest float32 implementation (EmuBackend, and for Adam a float32
evaluation of the C ABI's contract) inside the bound at EVERY case the GPU test runs; and the mutations a subtly wrong
kernel makes, each outside the bound in at least one case of the same tables."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emu_backend
import head_ref64 as H
from emu_backend import EmuBackend

D = torch.float64


class Honest(H.AbiAdam, EmuBackend):
    pass


def _accepts(vs):
    assert not H.failures(vs), H.failures(vs)[:4]


# ----------------------------------------------------------------------------- the restatements against torch float64
@pytest.mark.parametrize("k,dims,rate", [((4, 2, 2), (6, 4, 4), 0.0), ((4, 2, 2), (6, 4, 4), 0.5), ((2, 3, 3), (2, 3, 3), 0.5)])
def test_ref64_head_pool_matches_avg_pool3d_and_autograd(k, dims, rate):
    g0 = torch.Generator().manual_seed(0)
    n, c = 2, 12
    x = torch.randn(n, c, *dims, dtype=D, generator=g0, requires_grad=True)
    P = int(np.prod(H.positions(dims, k)))
    keep = torch.from_numpy(emu_backend.keep_mask(77, n, c, 5, P, rate))
    pooled = F.avg_pool3d(x, k, stride=1).reshape(n, c, P)
    feat = (pooled * keep / (1.0 - rate)).mean(2)
    g = torch.randn(n, c, dtype=D, generator=g0)
    feat.backward(g)
    r, a = H.head_pool_fwd(x.detach().permute(0, 2, 3, 4, 1), k, keep, rate)
    assert torch.allclose(r, feat.detach(), rtol=1e-12, atol=1e-12) and (a >= r.abs() - 1e-12).all()
    dx, da = H.head_pool_bwd(g, dims, k, keep, rate)
    assert torch.allclose(dx, x.grad.permute(0, 2, 3, 4, 1), rtol=1e-12, atol=1e-12) and (da >= dx.abs() - 1e-12).all()


def test_ref64_linear_matches_f_linear_and_autograd():
    g0 = torch.Generator().manual_seed(1)
    n, f, k = 5, 70, 11
    feat = torch.randn(n, f, dtype=D, generator=g0, requires_grad=True)
    w = torch.randn(k, f, dtype=D, generator=g0, requires_grad=True)
    b = torch.randn(k, dtype=D, generator=g0, requires_grad=True)
    out = F.linear(feat, w, b)
    dl = torch.randn(n, k, dtype=D, generator=g0)
    out.backward(dl)
    r, a = H.fc_fwd(feat.detach(), w.detach(), b.detach())
    assert torch.allclose(r, out.detach(), rtol=1e-12, atol=1e-12) and (a >= r.abs() - 1e-12).all()
    assert torch.allclose(H.fc_fwd(feat.detach(), w.detach(), None)[0], F.linear(feat, w).detach(), rtol=1e-12, atol=1e-12)
    dw_in, db_in = torch.randn(k, f, dtype=D, generator=g0), torch.randn(k, dtype=D, generator=g0)
    (rf, _), (rw, _), (rb, _) = H.fc_bwd(dl, feat.detach(), w.detach(), dw_in, db_in)
    assert torch.allclose(rf, feat.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rw, dw_in + w.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb, db_in + b.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k,kind", [(11, "sd1"), (257, "sd40"), (600, "neginf"), (7, "equal")])
def test_ref64_softmax_ce_matches_cross_entropy_and_autograd(k, kind):
    g0 = torch.Generator().manual_seed(2)
    n = 5
    x32, labels = H.ce_logits(k, n, kind, g0)
    x = x32.double().requires_grad_(True)
    loss = F.cross_entropy(x, labels)
    loss.backward()
    ref = H.softmax_ce(x32, labels, 0.5)
    assert torch.allclose(ref["dl"], x.grad * 0.5, rtol=1e-12, atol=1e-12)
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert (ref["a"] >= ref["dl"].abs() - 1e-15).all()


def test_ref64_softmax_ce_counts_the_first_maximum():
    x, labels = H.ce_tie_logits(torch.Generator().manual_seed(3))
    ref = H.softmax_ce(x, labels, 1.0)
    assert ref["correct"] == sum(1 for i, _, lab in H.CE_TIES if lab == i) == 3


@pytest.mark.parametrize("step0", [0, 1, 9999])
def test_ref64_adam_matches_torch_optim_adam_in_float64(step0):
    g0 = torch.Generator().manual_seed(4)
    p0, g, m, v, _ = (x.double() if torch.is_tensor(x) else x for x in H.adam_inputs(513, step0, g0))
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=H.ADAM_LR, betas=H.ADAM_BETAS, eps=H.ADAM_EPS, foreach=False)
    opt.state[tp] = dict(step=torch.tensor(float(step0)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    tp.grad = g * 0.5
    opt.step()
    r = H.adam_ref(p0, g, m, v, step0 + 1, H.ADAM_LR, *H.ADAM_BETAS, H.ADAM_EPS, 0.5, abi=False)
    st = opt.state[tp]
    assert torch.allclose(r["m"], st["exp_avg"], rtol=1e-12, atol=1e-300)
    assert torch.allclose(r["v"], st["exp_avg_sq"], rtol=1e-12, atol=1e-300)
    assert torch.allclose(r["p"], tp.detach(), rtol=1e-12, atol=1e-300)
    # the float ABI: 1 - float32(0.999) is not float32(0.001) -- v's increment differs by 1.3e-5 relative, by contract
    ra = H.adam_ref(p0, g, m, v, step0 + 1, H.ADAM_LR, *H.ADAM_BETAS, H.ADAM_EPS, 0.5, abi=True)
    inc, inc_a = r["v"] - 0.999 * v, ra["v"] - H.f32(0.999) * v
    nz = g != 0
    rel = ((inc_a - inc).abs() / inc.abs().clamp_min(1e-300))[nz].max()
    assert 1.0e-5 < float(rel) < 1.6e-5, float(rel)


# ----------------------------------------------------------------------------- honest float32 is inside the bound, everywhere
@pytest.mark.parametrize("case", H.POOL_CASES, ids=[c["name"] for c in H.POOL_CASES])
def test_honest_float32_head_pool_is_inside_the_bound(case):
    _accepts(H.check_pool(Honest(), "cpu", case))


@pytest.mark.parametrize("case", H.FC_CASES, ids=[f"n{c[0]}-f{c[1]}-k{c[2]}" for c in H.FC_CASES])
def test_honest_float32_linear_is_inside_the_bound(case):
    for mode, bias in H.FC_MODES:
        _accepts(H.check_fc(Honest(), "cpu", case, mode, bias))


@pytest.mark.parametrize("k", H.CE_K)
def test_honest_float32_softmax_ce_is_inside_the_bound(k):
    worst = 0.0
    for case in (c for c in H.CE_CASES if c[0] == k):
        vs = H.check_ce(Honest(), "cpu", case)
        worst = max(worst, H.worst_of(vs))
        _accepts(vs)
    print(f"k {k}: honest float32 worst error/bound {worst:.3g}")


def test_honest_float32_softmax_ce_ties_are_inside_the_bound():
    _accepts(H.check_ce_ties(Honest(), "cpu"))


@pytest.mark.parametrize("count", H.ADAM_COUNTS)
def test_honest_float32_adam_is_inside_the_bound(count):
    worst = 0.0
    for step0, gscale, shadow in H.adam_cases(count):
        vs, _ = H.check_adam(Honest(), "cpu", count, step0, gscale, shadow, with_torch=count != H.ADAM_BIG)
        worst = max(worst, H.worst_of(vs))
        _accepts(vs)
    print(f"count {count}: honest float32 worst error/bound {worst:.3g}")


def test_honest_float32_adam_split_is_bit_equal():
    for count, cut in ((4096 + 3, 4), (4096 + 3, 2048), (1023, 1020)):
        _accepts(H.check_adam_split(Honest(), "cpu", count, cut, 1, 0.5, H.BF16))


# ----------------------------------------------------------------------------- the terms the two bounds carry are needed
def test_softmax_bound_without_the_difference_term_refuses_honest_float32(monkeypatch):
    """ref64.compare as it stands, a = (p + onehot) / n: honest float32 softmax at widely spread logits is outside it"""
    orig = H.softmax_ce
    monkeypatch.setattr(H, "softmax_ce", lambda x, labels, gscale: orig(x, labels, gscale, diff_term=False))
    bad = [c for c in H.CE_CASES if c[3] == "sd40" and c[0] >= 249 and H.failures(H.check_ce(Honest(), "cpu", c))]
    assert bad


def test_adam_bound_without_the_propagated_term_refuses_honest_float32(monkeypatch):
    """elem_bound(p', |p| + |dp|, 4) alone: where m' cancels, its own rounding moves dp by more than 20 ulp of |dp|"""
    orig = H.adam_bounds

    def no_prop(r):
        bm, bv, a_p, prop = orig(r)
        return bm, bv, a_p, torch.zeros_like(prop)
    monkeypatch.setattr(H, "adam_bounds", no_prop)
    vs, _ = H.check_adam(Honest(), "cpu", 4096 + 3, 9999, 1.0, None, with_torch=False)
    assert [v for v in H.failures(vs) if v.name.startswith("p ")]


# ----------------------------------------------------------------------------- mutations: each outside the bound somewhere
def _rejected(check, cases):
    """True as soon as one case of the table refuses the mutant"""
    return any(H.failures(check(c)) for c in cases)


def _patch_keep(monkeypatch, fn):
    orig = emu_backend.keep_mask
    monkeypatch.setattr(emu_backend, "keep_mask", lambda seed, n, c, f_off, P, rate: fn(orig, seed, n, c, f_off, P, rate))


def test_mutant_keep_mask_without_f_off_is_rejected(monkeypatch):
    _patch_keep(monkeypatch, lambda orig, seed, n, c, f_off, P, rate: orig(seed, n, c, 0, P, rate))
    pairs = [c for c in H.POOL_CASES if len(c["parts"]) == 2]
    assert pairs and all(H.failures(H.check_pool(EmuBackend(), "cpu", c)) for c in pairs)


def test_mutant_keep_mask_of_channel_minus_256_is_rejected(monkeypatch):
    def wrapped(orig, seed, n, c, f_off, P, rate):
        m = orig(seed, n, c, f_off, P, rate).copy()
        if c > 256:
            m[:, 256:] = m[:, : c - 256].copy()
        return m
    _patch_keep(monkeypatch, wrapped)
    wide = [c for c in H.POOL_CASES if c["rate"] > 0 and c["parts"][0]["c"] > 256]
    assert wide and all(H.failures(H.check_pool(EmuBackend(), "cpu", c)) for c in wide)
    narrow = [c for c in H.POOLG_CASES]
    assert not any(H.failures(H.check_pool(EmuBackend(), "cpu", c)) for c in narrow)      # the mutation is what is seen


def test_mutant_forward_and_backward_masks_from_different_seeds_is_rejected():
    class M(EmuBackend):
        def head_pool_bwd(self, dfeat, feat_ld, f_off, k, rate, seed, dx):
            return super().head_pool_bwd(dfeat, feat_ld, f_off, k, rate, seed + 1, dx)
    drop = [c for c in H.POOL_CASES if c["rate"] > 0]
    assert all(H.failures(H.check_pool(M(), "cpu", c)) for c in drop)


def test_mutant_mean_without_the_slice_remainder_is_rejected():
    class M(EmuBackend):
        def head_pool_fwd(self, x, k, rate, seed, feat, feat_ld, f_off):
            sl = 32 if x.dtype == torch.bfloat16 else 16
            pixels = x.t * x.h * x.w
            use = pixels - pixels % sl
            if tuple(k) != (x.t, x.h, x.w) or use in (0, pixels):
                return super().head_pool_fwd(x, k, rate, seed, feat, feat_ld, f_off)

            def run(stream):
                v = x.view5().float().reshape(x.n, pixels, x.c)[:, :use].mean(1)
                if rate > 0:
                    keep = torch.from_numpy(emu_backend.keep_mask(int(seed[0]), x.n, x.c, f_off, 1, rate))[:, :, 0]
                    v = v * keep / (1.0 - rate)
                feat[: x.n * feat_ld].view(x.n, feat_ld)[:, f_off:f_off + x.c] = v
            return run
    rem = [c for c in H.POOL1_CASES if c["parts"][0]["dims"] == (4, 7, 7)]
    assert rem and all(H.failures(H.check_pool(M(), "cpu", c)) for c in rem)


def _fc_all(be):
    return lambda c: [v for mode, bias in H.FC_MODES for v in H.check_fc(be, "cpu", c, mode, bias)]


def test_mutant_dw_overwritten_is_rejected():
    class M(EmuBackend):
        def fc_bwd(self, dlogits, feat, w, dfeat, dw, db, n, f, k):
            run = super().fc_bwd(dlogits, feat, w, dfeat, dw, db, n, f, k)

            def r(stream):
                if dw is not None:
                    dw.zero_()
                if db is not None:
                    db.zero_()
                run(stream)
            return r
    assert all(H.failures(_fc_all(M())(c)) for c in H.FC_CASES)


def test_mutant_bias_dropped_is_rejected():
    class M(EmuBackend):
        def fc_fwd(self, feat, w, b, logits, n, f, k):
            return super().fc_fwd(feat, w, None, logits, n, f, k)
    assert all(H.failures(_fc_all(M())(c)) for c in H.FC_CASES)


def test_mutant_softmax_without_max_subtraction_fails_at_the_shift():
    class M(EmuBackend):
        def softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct):
            def run(stream):
                lg = logits.reshape(-1)[: n * k].view(n, k)
                e = lg.exp()
                p = e / e.sum(1, keepdim=True)
                loss = (e.sum(1).log() - lg[torch.arange(n), labels[:n]]).sum() / n
                if dlogits is not None:
                    d = p.clone()
                    d[torch.arange(n), labels[:n]] -= 1
                    dlogits.reshape(-1)[: n * k].copy_((d / n * gscale).reshape(-1))
                for acc in (loss_out, loss_sum):
                    if acc is not None:
                        acc[0] += loss
                if correct is not None:
                    correct[0] += int((lg.argmax(1) == labels[:n]).sum())
            return run
    shifted = [c for c in H.CE_CASES if c[3] == "shift3e4"]
    for c in shifted:                                   # inf / nan must be a failure, never a pass
        vs = H.check_ce(M(), "cpu", c)
        assert [v for v in H.failures(vs) if v.name.startswith("dlogits k")], c
        assert [v for v in H.failures(vs) if v.name.startswith("loss")], c
    assert not any(H.failures(H.check_ce(M(), "cpu", c)) for c in H.CE_CASES if c[3] == "sd1")


def test_mutant_tie_resolved_to_the_last_index_is_rejected():
    class M(EmuBackend):
        def softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct):
            run = super().softmax_ce(logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, None)

            def r(stream):
                run(stream)
                if correct is not None:
                    lg = logits.reshape(-1)[: n * k].view(n, k)
                    last = k - 1 - lg.flip(1).argmax(1)
                    correct[0] += int((last == labels[:n]).sum())
            return r
    bad = H.failures(H.check_ce_ties(M(), "cpu"))
    assert {v.name for v in bad} >= {f"correct tie-row{r}" for r in range(len(H.CE_TIES))} | {"correct ties"}, bad
    assert all(v.name.startswith("correct") for v in bad)


def test_mutant_gscale_ignored_in_the_loss_gradient_is_rejected():
    class M(EmuBackend):
        def softmax_ce(self, logits, labels, n, k, gscale, dlogits, loss_out, loss_sum, correct):
            return super().softmax_ce(logits, labels, n, k, 1.0, dlogits, loss_out, loss_sum, correct)
    scaled = [c for c in H.CE_CASES if c[2] != 1.0 and c[0] > 1]
    assert all(H.failures(H.check_ce(M(), "cpu", c)) for c in scaled)
    assert not any(H.failures(H.check_ce(M(), "cpu", c)) for c in H.CE_CASES if c[2] == 1.0)


def _adam_mutant(**attrs):
    return type("M", (Honest,), attrs)()


def _adam_rejected(be, counts, pick=lambda case: True):
    out = []
    for count in counts:
        for case in filter(pick, H.adam_cases(count)):
            vs, _ = H.check_adam(be, "cpu", count, *case, with_torch=False)
            out.append(bool(H.failures(vs)))
    return out


SMALL = [c for c in H.ADAM_COUNTS if c != H.ADAM_BIG]


def test_mutant_adam_bias_correction_with_step_minus_one_is_rejected():
    # (at step 10 000 both corrections are 1 to within 5e-8: the mutation is invisible there, and harmless)
    assert all(_adam_rejected(_adam_mutant(step_off=1), SMALL, lambda case: case[0] != 9999))


def test_mutant_adam_without_eps_is_rejected():
    got = _adam_rejected(_adam_mutant(no_eps=True), [1023, 4096 + 1])
    assert all(got), got


def test_mutant_adam_gscale_on_g_but_not_on_g_squared_is_rejected():
    be = _adam_mutant(gscale_on_g_only=True)
    assert all(_adam_rejected(be, SMALL, lambda case: case[1] != 1.0))
    assert not any(_adam_rejected(be, [1023], lambda case: case[1] == 1.0))


def test_mutant_adam_without_the_last_count_mod_4_elements_is_rejected():
    be = _adam_mutant(skip_mod4_tail=True)
    assert all(_adam_rejected(be, [c for c in SMALL if c % 4]))
    assert not any(_adam_rejected(be, [4]))


def test_mutant_adam_that_stops_at_the_grid_cap_is_rejected():
    be = _adam_mutant(grid_cap=H.ADAM_GRID_CAP)
    assert all(_adam_rejected(be, [H.ADAM_BIG]))
    assert not any(_adam_rejected(be, [4096 + 3], lambda case: case == (9999, 0.5, H.BF16)))
