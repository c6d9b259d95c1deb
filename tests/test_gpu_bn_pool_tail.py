"""The kernels between the conv launches and the head on an MI355X, element by element against float64 (tests/bn_ref64.py):
sfk_bn_apply in all six RES x RELU forms with relu_bits and out_sums, sfk_bn_bwd_apply, sfk_bn_finalize / sfk_bn_eval_coeffs /
sfk_bn_bwd_finalize on seeded partial rows, sfk_maxpool_fwd / bwd at four windows, and sfk_bn_tail_fwd / bwd without convs.
The shapes are the smallest at which each kernel takes every one of its paths: one channel group, 25 rows per block with idle
threads, one full 256-group chunk and a partial second one; 1 pixel, fewer pixels than a block has rows, and every remainder of
the last 4-row span; the out_sums grid-stride loop on 1 / 3 / uncapped blocks; 1 .. 50,176 partial rows with and without the
fold workspace; tail shapes that stop inside every tile and fill the second register column partly and fully.  Three large
launches hold the loops no small case reaches: both apply kernels across the 65,535-block grid cap (one launch bit for bit
against two halves) and the streamed sfk_bn_bwd_apply of maps above sfk_tuning.nt_bwd_apply_mb.
tests/test_bn_ref_cpu.py pins the same tables without a GPU: honest float32 inside every bound, the mutations outside.
Inputs are finite except the one NaN pool case; the refusal cases check only the status returned before any launch."""
import re

import pytest
import torch

import bn_ref64 as B

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GROUP_IDS = [f"{B.tag_of(d)}-{cm}groups" for d, cm in B.APPLY_GROUPS]


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    return HipBackend()


def report(vs, every: bool = True):
    print()
    for v in vs:
        if every or not v.ok:
            print(f"  {v}")
    print(f"  {len(vs)} verdicts, worst error/bound {B.worst_of(vs):.3g}")
    assert not B.failures(vs), B.failures(vs)[:8]


def run_table(hip, cases, check, name):
    vs = []
    for case in cases:
        got = check(hip, DEV, case)
        print(f"  {name(case)}: {len(got)} verdicts, worst error/bound {B.worst_of(got):.3g}"
              f"{'' if not B.failures(got) else ' FAIL'}")
        vs += got
    report(vs, every=False)


@pytest.mark.parametrize("dtype,cm", B.APPLY_GROUPS, ids=GROUP_IDS)
def test_bn_apply(hip, dtype, cm):
    run_table(hip, B.group_of(B.APPLY_CASES, dtype, cm), B.check_apply, B.case_name)


@pytest.mark.parametrize("dtype,cm", B.APPLY_GROUPS, ids=GROUP_IDS)
def test_bn_apply_out_sums(hip, dtype, cm):
    run_table(hip, B.group_of(B.SUMS_CASES, dtype, cm), B.check_apply, B.case_name)


@pytest.mark.parametrize("dtype,cm", B.APPLY_GROUPS, ids=GROUP_IDS)
def test_bn_bwd_apply(hip, dtype, cm):
    run_table(hip, B.group_of(B.BWD_APPLY_CASES, dtype, cm), B.check_bwd_apply, B.case_name)


@pytest.mark.parametrize("c", sorted({c["c"] for c in B.FIN_CASES}))
def test_bn_finalize_and_bwd_finalize(hip, c):
    run_table(hip, [k for k in B.FIN_CASES if k["c"] == c], B.check_finalize, B.fin_name)


@pytest.mark.parametrize("c", B.EVAL_C)
def test_bn_eval_coeffs(hip, c):
    report(B.check_eval_coeffs(hip, DEV, c))


def _refused(run, status: int):
    from video_classification_amd._lib import SfkError
    with pytest.raises(SfkError, match=re.escape(f"({status})")):
        run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_finalize_refusals_leave_every_output_untouched(hip):
    """an odd channel count is SFK_ERR_UNSUPPORTED (-2), partial rows off 16-byte alignment SFK_ERR_INVALID (-1): both are
    returned before any launch, so nothing is written"""
    for c, shift_, status in ((3, 0, -2), (6, 2, -1)):
        parts = torch.randn(8 * c * 2 + 4, device=DEV)
        gamma, beta, invstd_in = (torch.rand(c, device=DEV) + 0.5 for _ in range(3))
        outs = [torch.full((c * 3 + B.GUARD,), B.SENT, device=DEV) for _ in range(9)]
        mean, invstd, scale, shift, rm, rv, dgamma, dbeta, coef = outs
        nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
        p = parts[shift_:]
        _refused(hip.bn_finalize(p, 8, c, 32, gamma, beta, B.EPS, B.MOMENTUM, rm, rv, nbt, mean, invstd, scale, shift), status)
        _refused(hip.bn_bwd_finalize(p, 8, c, 32, gamma, invstd_in, dgamma, dbeta, coef), status)
        assert int(nbt[0]) == 41 and all(bool((o == B.SENT).all()) for o in outs), (c, shift_)


def test_tail_refuses_more_than_512_input_channels(hip):
    """c = 513 is SFK_ERR_UNSUPPORTED before the fold of g or anything else is launched"""
    c, cout = 513, 8
    z = lambda n: torch.zeros(n, device=DEV)
    outs = [torch.full((n,), B.SENT, device=DEV) for n in (c, cout, cout, cout, cout, cout * c, c * cout, cout, cout)]
    g, mean, invstd, scale, shift, t, wd, rm, rv = outs
    nbt = torch.tensor([41], dtype=torch.int64, device=DEV)
    _refused(hip.bn_tail_fwd(z(c * c), z(c * 2), 1, 16, g, c, z(cout * c), cout, z(cout), z(cout), B.EPS, B.MOMENTUM, rm, rv, nbt,
                             mean, invstd, scale, shift, t, wd), -2)
    assert int(nbt[0]) == 41 and all(bool((o == B.SENT).all()) for o in outs)


@pytest.mark.parametrize("dtype", [B.BF16, B.F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("window", B.POOL_WINDOWS, ids=[f"k{k}s{s}p{p}" for k, s, p in B.POOL_WINDOWS])
def test_maxpool(hip, dtype, window):
    cases = [c for c in B.POOL_CASES if c["dtype"] == dtype and (c["k"], c["s"], c["p"]) == window]
    run_table(hip, cases, B.check_pool, B.pool_name)


@pytest.mark.parametrize("shape", B.TAIL_SHAPES, ids=[f"c{c}-cout{co}" for c, co in B.TAIL_SHAPES])
def test_bn_tail(hip, shape):
    run_table(hip, [c for c in B.TAIL_CASES if (c["c"], c["cout"]) == shape and not c["md"]], B.check_tail, B.tail_name)


def test_bn_tail_mean_dominated_channels(hip):
    report(B.check_tail(hip, DEV, next(c for c in B.TAIL_CASES if c["md"])))


def test_bn_apply_across_the_grid_cap(hip):
    """fp32, 1024 channels, 4 * 65535 + 1030 pixels (1.07 GB per map): the second trip of the span loop"""
    try:
        report(B.check_grid_cap_apply(hip, DEV))
    finally:
        torch.cuda.empty_cache()


def test_bn_bwd_apply_across_the_grid_cap(hip):
    try:
        report(B.check_grid_cap_bwd_apply(hip, DEV))
    finally:
        torch.cuda.empty_cache()


def test_bn_bwd_apply_streamed(hip):
    """the non-temporal instantiation production runs on its large maps: bf16, 64 channels, the first pixel count at the
    threshold plus 37"""
    from video_classification_amd._lib import tuning
    mb = int(tuning().nt_bwd_apply_mb)
    assert 0 < mb <= 512, mb
    px = B.streamed_px(mb)
    assert px * B.STREAM_C * 2 >= mb << 20 > (px - 38) * B.STREAM_C * 2
    try:
        report(B.check_streamed_bwd_apply(hip, DEV, px))
    finally:
        torch.cuda.empty_cache()
