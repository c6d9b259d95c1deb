"""Everything after the last bottleneck on an MI355X, element by element against float64 (tests/head_ref64.py):
sfk_head_pool_fwd / bwd with sfk_head_dropout_mask, sfk_fc_fwd / bwd, sfk_softmax_ce, sfk_adam, and sfk_sgd across the
grid cap.  The shapes are the smallest at which each kernel takes every one of its paths: a second, partial 256-channel
block, a second channel-group block of the backward, a pixel-slice remainder, a strided map, the two-pathway pairing into
one feat; accumulation onto non-zero dw / db and the engine's split launch; softmax rows longer than the block with ties,
shifted and -inf logits; Adam counts around the vector width and across the capped grid, with both shadows and the split
form.  tests/test_head_opt_ref_cpu.py pins the same tables without a GPU: honest float32 inside every bound, the mutations
outside.  Labels stay in range and no logit is NaN: sfk_softmax_ce indexes logits[label] unchecked."""
import pytest
import torch

import head_ref64 as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    return HipBackend()


def report(vs):
    print()
    for v in vs:
        print(f"  {v}")
    print(f"  worst error/bound {H.worst_of(vs):.3g}")
    assert not H.failures(vs), H.failures(vs)


@pytest.mark.parametrize("case", H.POOL1_CASES, ids=[c["name"] for c in H.POOL1_CASES])
def test_head_pool_single_position(hip, case):
    report(H.check_pool(hip, DEV, case))


@pytest.mark.parametrize("case", H.POOLG_CASES, ids=[c["name"] for c in H.POOLG_CASES])
def test_head_pool_general(hip, case):
    vs = H.check_pool(hip, DEV, case)
    assert any(v.name.startswith("mask ") for v in vs)          # the mask kernel's bits against keep_mask
    report(vs)


@pytest.mark.parametrize("case", H.FC_CASES, ids=[f"n{c[0]}-f{c[1]}-k{c[2]}" for c in H.FC_CASES])
def test_linear(hip, case):
    vs = []
    for mode, bias in H.FC_MODES:
        vs += H.check_fc(hip, DEV, case, mode, bias)
    report(vs)


@pytest.mark.parametrize("k", H.CE_K)
def test_softmax_ce(hip, k):
    vs = []
    for case in (c for c in H.CE_CASES if c[0] == k):
        vs += H.check_ce(hip, DEV, case)
    report(vs)


def test_softmax_ce_counts_the_first_maximum(hip):
    report(H.check_ce_ties(hip, DEV))


@pytest.mark.parametrize("count", H.ADAM_COUNTS)
def test_adam(hip, count):
    vs, dist = [], 0.0
    for step0, gscale, shadow in H.adam_cases(count):
        v, d = H.check_adam(hip, DEV, count, step0, gscale, shadow)
        vs += v
        dist = max(dist, d)
    report(vs)
    print(f"  count {count}: kernel to torch.optim.Adam(foreach=False), worst {dist:.3g} ulp of the updated p")


@pytest.mark.parametrize("count,cut", [(4096 + 3, 4), (4096 + 3, 2048), (1023, 1020), (H.ADAM_BIG, 1024)])
def test_adam_split_is_bit_equal_to_one_launch(hip, count, cut):
    vs = []
    for step0, shadow in ((0, None), (9999, H.BF16)):
        vs += H.check_adam_split(hip, DEV, count, cut, step0, 0.5, shadow)
    report(vs)


@pytest.mark.parametrize("cut", [1, 2, 3, 6])
def test_adam_refuses_a_cut_that_is_no_multiple_of_4(hip, cut):
    """the vector path needs 16-byte pointers: SFK_ERR_UNSUPPORTED from the entry point, before any launch"""
    from video_classification_amd._lib import SfkError
    count = 4096
    p, g, m, v = (torch.full((count,), 0.5, device=DEV) for _ in range(4))
    step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    run = hip.adam(p[cut:], g[cut:], m[cut:], v[cut:], count - cut, H.ADAM_LR, *H.ADAM_BETAS, H.ADAM_EPS, 1.0, step, None)
    with pytest.raises(SfkError, match="unsupported"):
        run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(step[0]) == 3 and all(bool((x == 0.5).all()) for x in (p, g, m, v))


def within_ulp(a, b, scale):
    """|a - b| <= 1 ulp of `scale` (tests/test_gpu_v2.py: torch's add(alpha=) fuses its multiply-add, sfk_sgd rounds the
    product first)"""
    return bool(((a - b).abs() <= torch.finfo(torch.float32).eps * scale.abs()).all())


def test_sgd_across_the_grid_cap(hip):
    """sfk_sgd at 16384 * 1024 + 1029 elements -- the capped grid's second trip and the scalar tail, which the v2 arena
    takes every step -- checked as test_sgd_matches_torch checks 1 M: two steps (the first and a later one), Nesterov"""
    count, lr, mom, gs, damp, nesterov = H.ADAM_BIG, 0.05, 0.9, 0.5, 0.0, True
    g0 = torch.Generator(device=DEV).manual_seed(9)
    p = torch.randn(count, generator=g0, device=DEV)
    buf = torch.zeros(count, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    shadow = torch.empty(count, dtype=torch.bfloat16, device=DEV)
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=mom, dampening=damp, nesterov=nesterov, foreach=False)
    for k in range(2):
        g = torch.randn(count, generator=g0, device=DEV)
        p0, b0 = p.clone(), buf.clone()
        hip.sgd(p, g, buf, count, lr, mom, damp, nesterov, gs, step, shadow)(torch.cuda.current_stream().cuda_stream)
        tp.grad = g * gs
        opt.step()
        torch.cuda.synchronize()
        assert int(step[0]) == k + 1
        tb = opt.state[tp]["momentum_buffer"]
        bterms = (g * gs).abs() if k == 0 else (mom * b0).abs() + ((1 - damp) * g * gs).abs()
        d = (g * gs).abs() + mom * tb.abs()
        assert within_ulp(buf, tb, bterms) and within_ulp(p, tp.detach(), p0.abs() + lr * d), k
        assert torch.equal(shadow, p.to(torch.bfloat16))
        with torch.no_grad():
            tp.copy_(p)
            opt.state[tp]["momentum_buffer"].copy_(buf)
