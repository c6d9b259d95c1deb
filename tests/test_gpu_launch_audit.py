"""Every conv / stem / BatchNorm launch the default bf16 train plans bind at the production geometries, replayed once on
seeded buffers and held to a float64 bound per element (tests/launch_audit.py, tests/ref64.py):
  * bench: SlowFast-R50 8x8, N 32, 3 x 32 x 224^2, slow pathway through pack_pathway_index;
  * res2d.yaml: ResNet-50 over stacked frames, N 60, T 10, 128^2;
  * v2: SlowFast-R50, N 10, T 20, 192^2, input channels (5, 2).
The replayed descriptor must report the family the plan bound, so the route audited is the route the bench runs.  The
stem tail is also chained at the bench size (forward, backward reduce, finalize, apply) with dgamma / dbeta checked
against float64 sums taken directly from d_out."""
import collections
import time

import pytest
import torch

import launch_audit as la
import ref64
from ref64 import F64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def test_production_plan_launches_match_float64():
    from video_classification_amd._lib import HipBackend
    be = HipBackend()
    t0 = time.time()
    rec = la.record_plans(be, DEV, la.PRODUCTION)
    torch.cuda.empty_cache()
    sigs = sorted(rec.calls, key=lambda s: (s[0], la.describe(s)))
    print(f"\nrecorded {len(sigs)} distinct launches in {time.time() - t0:.1f} s")
    per_kind = collections.Counter()
    per_geo = collections.Counter()
    fams = collections.Counter()
    worst = collections.defaultdict(float)
    failed, fam_bad = [], []
    t1 = time.time()
    for i, s in enumerate(sigs):
        r = la.replay(s, be, DEV, seed=i)
        tags = ",".join(sorted(rec.calls[s]))
        per_kind[s[0]] += 1
        for t in rec.calls[s]:
            per_geo[(t, s[0])] += 1
        if s[3] is not None:
            fams[s[3]] += 1
            if r.family != s[3]:
                fam_bad.append((la.describe(s), s[3], r.family))
        worst[s[0]] = max(worst[s[0]], r.worst)
        detail = r.ok and all(v.kind != "bits" for v in r.verdicts)
        print(f"{'ok  ' if r.ok else 'FAIL'} {la.describe(s)} fam {s[3]} [{tags}] worst {r.worst:.3g} "
              f"agg/bound {r.agg:.3g}" + ("" if detail else f" {r.verdicts} untouched-bad {r.untouched_bad}"))
        if not r.ok:
            failed.append(la.describe(s))
        torch.cuda.empty_cache()
    print(f"replayed {len(sigs)} launches in {time.time() - t1:.1f} s")
    for k in sorted(per_kind):
        print(f"  {k}: {per_kind[k]} signatures, worst error/bound {worst[k]:.3g}, "
              + ", ".join(f"{g} {per_geo[(g, k)]}" for g in la.PRODUCTION if per_geo[(g, k)]))
    print("  conv families: " + ", ".join(f"{f}: {n}" for f, n in sorted(fams.items())))
    assert not fam_bad, fam_bad
    assert {1, 4, 5} <= set(fams), fams
    assert all(tags for tags in rec.calls.values())
    assert not failed, failed


def test_stem_tail_chain_at_the_bench_size():
    """BatchNorm -> ReLU -> MaxPool of the fast stem at N 32 (12.8 M pixels x 8 channels), forward then backward reduce,
    finalize and apply, chained as the plan runs them; dgamma / dbeta against float64 sums taken from d_out"""
    from video_classification_amd._lib import FMap, HipBackend
    be = HipBackend()
    g = torch.Generator(device=DEV).manual_seed(11)
    n, t, h, w, c = 32, 32, 112, 112, 8
    y = FMap(torch.randn(n * t * h * w * c, generator=g, device=DEV).to(torch.bfloat16), n, t, h, w, c)
    yv = y.view5().to(F64).reshape(-1, c)
    mean64, var64 = yv.mean(0), yv.var(0, unbiased=False)
    mean, invstd = mean64.float(), (1.0 / torch.sqrt(var64 + 1e-5)).float()
    gamma = torch.randn(c, generator=g, device=DEV)
    beta = torch.randn(c, generator=g, device=DEV)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    out = FMap(torch.empty(n * t * 56 * 56 * c, dtype=torch.bfloat16, device=DEV), n, t, 56, 56, c)
    argmax = torch.empty(out.pixels * c, dtype=torch.uint8, device=DEV)
    be.bn_maxpool_fwd(y, scale, shift, out, argmax, 3, 2, 1)(0)
    d_out = FMap(torch.randn(out.pixels * c, generator=g, device=DEV).to(torch.bfloat16), n, t, 56, 56, c)
    max_parts = 4096
    parts = torch.empty(max_parts * c * 2, device=DEV)
    run, np_ = be.bn_maxpool_bwd_reduce(d_out, argmax, y, mean, invstd, scale, shift, parts, max_parts)
    run(0)
    dgamma, dbeta = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    coef = torch.empty(c * 3, device=DEV)
    ws = torch.empty(64 * c * 2, device=DEV)
    be.bn_bwd_finalize(parts, np_, c, y.pixels, gamma, invstd, dgamma, dbeta, coef, ws)(0)
    da_map = FMap(torch.empty(y.pixels * c, dtype=torch.bfloat16, device=DEV), n, t, h, w, c)
    be.bn_maxpool_bwd_apply(d_out, argmax, y, mean, invstd, scale, shift, coef, da_map)(0)
    torch.cuda.synchronize()

    # float64: the forward from y, the kernel's argmax checked against it, the gradients taken straight from d_out
    v, vb = ref64.bn_pre(y.view5(), scale, shift)
    act = ref64.rounded(v.clamp_min(0), torch.bfloat16)
    best, _ = ref64.maxpool_fwd(act, 3, 2, 1)
    assert torch.equal(out.view5().to(F64), best)
    arg = argmax.view(n, t, 56, 56, c)
    da = ref64.rounded(ref64.maxpool_bwd(d_out.view5(), arg, h, w, 3, 2, 1), torch.bfloat16)
    m, amb = v > 0, v.abs() <= vb
    dz = (da * m).reshape(-1, c)
    xh = ((y.view5().to(F64) - mean.to(F64)) * invstd.to(F64)).reshape(-1, c)
    db64, dg64 = dz.sum(0), (dz * xh).sum(0)
    a_b = (da.abs() * (m | amb)).reshape(-1, c).sum(0)
    a_g = (da.abs() * (m | amb)).reshape(-1, c).mul(xh.abs() + 1e-30).sum(0)
    P = y.pixels
    vb_ = ref64.compare("dbeta", dbeta, db64, a_b, P, torch.float32, "sum_f32")
    vg_ = ref64.compare("dgamma", dgamma, dg64, a_g, P, torch.float32, "sum_f32")
    rb = float(((dbeta.double() - db64).norm() / db64.norm()))
    rg = float(((dgamma.double() - dg64).norm() / dg64.norm()))
    print(f"\nstem tail N {n}: nparts {np_}; dbeta rel-l2 {rb:.3g} ({vb_}); dgamma rel-l2 {rg:.3g} ({vg_})")
    print(f"  ambiguous ReLU signs {int(amb.sum())} of {amb.numel()}; |dbeta| {db64.abs().tolist()}")
    cf = coef.view(c, 3).double()
    r = cf[:, 0] * (dz - cf[:, 1] - xh * cf[:, 2])
    ar = cf[:, 0].abs() * (dz.abs() + cf[:, 1].abs() + xh.abs() * cf[:, 2].abs())
    alt = cf[:, 0] * ((da * ~m).reshape(-1, c) - cf[:, 1] - xh * cf[:, 2])
    vd = ref64.compare("dy", da_map.view5().reshape(-1, c), r, ar, 4, torch.bfloat16, "map_bf16", alt=alt,
                       alt_mask=amb.reshape(-1, c))
    print(f"  {vd}")
    assert vb_.ok and vg_.ok and vd.ok
