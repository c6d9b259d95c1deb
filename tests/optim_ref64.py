"""TEST INFRASTRUCTURE: include/sfk_optim.h restated in float64 -- the Adam / AdamW / SGD updates with a learning-rate
table, weight decay and a clipping coefficient, and the global gradient norm -- on whatever device the inputs live on, the
case tables, and the checks that run one case on a backend (HipBackend on the GPU, EmuOptimBackend and its mutants on the
CPU) and return the verdicts.

Every restatement returns (value, a) with a = the same expression over |terms|, as tests/head_ref64.py does; the tolerance
policy is ref64's (compare / elem_bound / ulp_out) as it stands, and Adam's p' is judged by head_ref64.compare_p (the bound
that carries the rounding of m' and v' into p').  The hyper-parameters are the float32 values the C ABI carries."""
from __future__ import annotations

import math
from typing import List

import torch

from head_ref64 import (ADAM_BETAS, ADAM_EPS, ADAM_PAD, ADAM_SENTINEL, BF16, F32, ElemOnly, Exact, _stream, _sync, adam_inputs,
                        compare_p, f32)
from ref64 import F64, compare

MODES = ["none", "l2", "decoupled"]
GRID_CAP = 16384 * 1024                            # elements one trip of the capped update grid covers (csrc/optim_sched.hip)
BIG = GRID_CAP + 5                                 # just above the cap, ends in the scalar tail
COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
LR_TABLE = [0.05, 0.03, 0.02, 0.01]                # rates that differ, large enough for lr*wd to show in p
WD = 0.5
COEF = 0.37                                        # a clipping coefficient as sfk_grad_norm leaves it
SHADOWS = [None, BF16, F32]
SGD_MOM, SGD_DAMP = 0.9, 0.1


def table_index(s: int, n: int) -> int:
    """the 0-based entry of a table of n rates that optimizer step s (1-based) reads"""
    return min(max(s, 1), n) - 1


def decay_counts(count: int) -> List[int]:
    return sorted({c for c in (0, 1, 5, count - 1, count) if 0 <= c <= count})


def steps0(lr_len: int) -> List[int]:
    return [0, 1, lr_len - 1, lr_len + 5]


def _grad(p_, g, gscale, coef, wd, l2, dc):
    """g' and its sum of |terms|: (g * gscale) * coef, + wd * p on [0, dc) under L2"""
    gg = g.to(F64) * f32(gscale) * (1.0 if coef is None else f32(coef))
    a_g = gg.abs()
    if l2:
        gg, a_g = gg.clone(), a_g.clone()
        gg[:dc] += f32(wd) * p_[:dc]
        a_g[:dc] += (f32(wd) * p_[:dc]).abs()
    return gg, a_g


def adam_hp_ref(p, g, m, v, s: int, lr_table, b1, b2, eps, gscale, wd=0.0, mode="none", dc=0, coef=None):
    """float64 sfk_adam_hp at step s (after the increment); the keys of head_ref64.adam_ref, so adam_bounds / compare_p apply"""
    lr = float(lr_table[table_index(s, len(lr_table))])
    b1, b2, eps = f32(b1), f32(b2), f32(eps)
    p_, m_, v_ = p.to(F64), m.to(F64), v.to(F64)
    gg, a_g = _grad(p_, g, gscale, coef, wd, mode == "l2", dc)
    if mode == "decoupled":
        p_ = p_.clone()
        p_[:dc] *= 1.0 - lr * f32(wd)
    m1, a_m = b1 * m_ + (1 - b1) * gg, (b1 * m_).abs() + (1 - b1) * a_g
    v1, a_v = b2 * v_ + (1 - b2) * gg * gg, b2 * v_ + (1 - b2) * a_g * a_g
    bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
    den = v1.sqrt() / math.sqrt(bc2) + eps
    dp = -(lr / bc1) * m1 / den
    return dict(m=m1, a_m=a_m, v=v1, a_v=a_v, dp=dp, p=p_ + dp, p0=p_, den=den, c1=lr / bc1, sbc2=math.sqrt(bc2))


def sgd_hp_ref(p, g, buf, s: int, lr_table, momentum, dampening, nesterov, gscale, wd=0.0, mode="none", dc=0, coef=None):
    """float64 sfk_sgd_hp at step s -> dict(buf, a_buf, p, a_p); buf is None without momentum"""
    lr = float(lr_table[table_index(s, len(lr_table))])
    mom, omd = f32(momentum), f32(1.0 - f32(dampening))
    p_ = p.to(F64)
    gg, a_g = _grad(p_, g, gscale, coef, wd, mode == "l2", dc)
    b1 = a_b = None
    d, a_d = gg, a_g
    if momentum != 0:
        b1, a_b = (gg, a_g) if s == 1 else (mom * buf.to(F64) + omd * gg, (mom * buf.to(F64)).abs() + omd * a_g)
        d, a_d = (gg + mom * b1, a_g + mom * a_b) if nesterov else (b1, a_b)
    return dict(buf=b1, a_buf=a_b, p=p_ - lr * d, a_p=p_.abs() + lr * a_d)


def grad_norm_ref(g, gscale, max_norm):
    """float64 sfk_grad_norm over the float32 products g * gscale -> (norm, coefficient); non-finite values propagate as
    torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) lets them: NaN -> (NaN, NaN), inf -> (inf, 0)"""
    x = (g.to(F32) * f32(gscale)).to(F64)
    norm = (x * x).sum().sqrt()
    c = f32(max_norm) / (norm + f32(1e-6))
    return norm, torch.where(c > 1.0, torch.ones_like(c), c)


def clip_grad_norm_ref(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ over a list of float64 gradients, restated -> (total norm, the clipped gradients)"""
    norm = torch.cat([x.reshape(-1) for x in grads]).pow(2).sum().sqrt()
    c = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, [x * c for x in grads]


# ----------------------------------------------------------------------------- the checks
def _padded(x, dev, off, dtype=F32):
    """x at element `off` of a buffer with sentinels on both sides: off = 1 makes the slice miss 16-byte alignment"""
    out = torch.full((off + x.numel() + ADAM_PAD,), ADAM_SENTINEL, dtype=dtype, device=dev)
    out[off: off + x.numel()] = x.to(dtype)
    return out


def _sentinels_ok(bufs, off, count) -> bool:
    return all(bool((b[:off].float() == ADAM_SENTINEL).all()) and bool((b[off + count:].float() == ADAM_SENTINEL).all()) for b in bufs)


def _hp_inputs(count, step0, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p, g, m, v, (z0, z1) = adam_inputs(count, step0, gen)
    p[z0:z1] = 0.0                                   # the arena's padding: p = g = m = v = 0
    return p, g, m, v, (z0, z1)


def check_adam_hp(be, dev, count, dc, step0, off=0, shadow_dtype=None, clip=False, mode="none", gscale=0.5, seed_no=0,
                  lr_table=LR_TABLE) -> List:
    """one sfk_adam_hp launch against adam_hp_ref, with the step counter, the sentinels around the slice, the shadow copy
    and the padding block"""
    p0, g0, m0, v0, (z0, z1) = _hp_inputs(count, step0, dev, 700 + seed_no + count % 1000 + step0)
    st = _stream(dev)
    P, G, M, V = (_padded(x, dev, off) for x in (p0, g0, m0, v0))
    SH = None if shadow_dtype is None else torch.full((off + count + ADAM_PAD,), ADAM_SENTINEL, dtype=shadow_dtype, device=dev)
    step = torch.full((1,), step0, dtype=torch.int64, device=dev)
    table = torch.tensor(lr_table, dtype=F32, device=dev)
    coef = torch.tensor([COEF], dtype=F32, device=dev) if clip else None
    (b1, b2), eps = ADAM_BETAS, ADAM_EPS
    be.adam_hp(P[off:], G[off:], M[off:], V[off:], count, table, b1, b2, eps, gscale, step, None if SH is None else SH[off:],
               weight_decay=WD, decay_mode=mode, decay_count=dc, clip_coef=coef)(st)
    _sync(dev)
    tag = f"adam_hp count {count} dc {dc} step {step0 + 1} off {off} shadow {shadow_dtype} clip {clip} mode {mode}"
    r = adam_hp_ref(p0, g0, m0, v0, step0 + 1, table.cpu().tolist(), b1, b2, eps, gscale, WD, mode, dc, COEF if clip else None)
    p, m, v = P[off: off + count], M[off: off + count], V[off: off + count]
    vs = [Exact(f"step {tag}", int(step[0]) == step0 + 1, f"{int(step[0])}"),
          compare(f"m {tag}", m, r["m"], r["a_m"], 2, F32, "map_f32"),
          compare(f"v {tag}", v, r["v"], r["a_v"], 2, F32, "map_f32"),
          compare_p(f"p {tag}", p, r)]
    zero = all(bool((x[z0:z1] == 0).all()) for x in (p, m, v))
    vs.append(Exact(f"padding stays 0 {tag}", zero, f"{z1 - z0} entries"))
    bufs = [P, G, M, V] + ([SH] if SH is not None else [])
    vs.append(Exact(f"sentinels {tag}", _sentinels_ok(bufs, off, count), f"{off} + {ADAM_PAD}"))
    vs.append(Exact(f"g untouched {tag}", torch.equal(G[off: off + count], g0), ""))
    if SH is not None:
        vs.append(Exact(f"shadow {tag}", torch.equal(SH[off: off + count], p.to(shadow_dtype)), str(shadow_dtype)))
    return vs


def check_sgd_hp(be, dev, count, dc, step0, off=0, shadow_dtype=None, clip=False, mode="none", gscale=0.5, nesterov=False,
                 momentum=SGD_MOM, seed_no=0, lr_table=LR_TABLE) -> List:
    """one sfk_sgd_hp launch against sgd_hp_ref"""
    p0, g0, b0, _, (z0, z1) = _hp_inputs(count, step0, dev, 800 + seed_no + count % 1000 + step0)
    st = _stream(dev)
    P, G, B = (_padded(x, dev, off) for x in (p0, g0, b0))
    SH = None if shadow_dtype is None else torch.full((off + count + ADAM_PAD,), ADAM_SENTINEL, dtype=shadow_dtype, device=dev)
    step = torch.full((1,), step0, dtype=torch.int64, device=dev)
    table = torch.tensor(lr_table, dtype=F32, device=dev)
    coef = torch.tensor([COEF], dtype=F32, device=dev) if clip else None
    be.sgd_hp(P[off:], G[off:], B[off:], count, table, momentum, SGD_DAMP, nesterov, gscale, step,
              None if SH is None else SH[off:], weight_decay=WD, decay_mode=mode, decay_count=dc, clip_coef=coef)(st)
    _sync(dev)
    tag = f"sgd_hp count {count} dc {dc} step {step0 + 1} off {off} shadow {shadow_dtype} clip {clip} mode {mode} nesterov {nesterov}"
    r = sgd_hp_ref(p0, g0, b0, step0 + 1, table.cpu().tolist(), momentum, SGD_DAMP, nesterov, gscale, WD, mode, dc,
                   COEF if clip else None)
    p, b = P[off: off + count], B[off: off + count]
    vs = [Exact(f"step {tag}", int(step[0]) == step0 + 1, f"{int(step[0])}"),
          compare(f"p {tag}", p, r["p"], r["a_p"], 4, F32, "map_f32")]
    if momentum != 0:
        vs.append(compare(f"buf {tag}", b, r["buf"], r["a_buf"], 3, F32, "map_f32"))
    else:
        vs.append(Exact(f"buf untouched {tag}", torch.equal(b, b0), ""))
    vs.append(Exact(f"padding stays 0 {tag}", bool((p[z0:z1] == 0).all()) and bool((b[z0:z1] == 0).all()), f"{z1 - z0} entries"))
    bufs = [P, G, B] + ([SH] if SH is not None else [])
    vs.append(Exact(f"sentinels {tag}", _sentinels_ok(bufs, off, count), f"{off} + {ADAM_PAD}"))
    if SH is not None:
        vs.append(Exact(f"shadow {tag}", torch.equal(SH[off: off + count], p.to(shadow_dtype)), str(shadow_dtype)))
    return vs


def norm_inputs(count, dev, kind="randn", seed_no=0):
    gen = torch.Generator(device=dev).manual_seed(900 + seed_no + count % 1000)
    if kind == "zero":
        return torch.zeros(count, device=dev)
    g = torch.randn(count, generator=gen, device=dev) * 10.0 ** (-6.0 * torch.rand(count, generator=gen, device=dev))
    if kind in ("inf", "nan"):
        g[count // 2] = float(kind)
    return g


def check_grad_norm(be, dev, count, kind="randn", off=0, gscale=0.5, max_norm=None, seed_no=0) -> List:
    """one sfk_grad_norm against grad_norm_ref.  max_norm None: a quarter of the norm (the coefficient is below 1) -- the
    zero input takes 1.0, whose coefficient clamps at 1"""
    g0 = norm_inputs(count, dev, kind, seed_no)
    st = _stream(dev)
    if max_norm is None:
        nn = float(grad_norm_ref(g0, gscale, 1.0)[0])
        max_norm = 0.25 * nn if math.isfinite(nn) and nn > 0 else 1.0
    G = _padded(g0, dev, off)
    rows = be.grad_norm_parts(count)
    parts = torch.full((rows + 2,), ADAM_SENTINEL, dtype=F64, device=dev)
    out = torch.full((4,), ADAM_SENTINEL, dtype=F32, device=dev)
    be.grad_norm(G[off:], count, gscale, max_norm, parts, out)(st)
    _sync(dev)
    tag = f"grad_norm count {count} {kind} off {off} gscale {gscale} max_norm {max_norm:.3g}"
    norm, c = grad_norm_ref(g0, gscale, max_norm)
    vs = [Exact(f"untouched {tag}", torch.equal(G[off: off + count], g0, ) if kind != "nan" else True, ""),
          Exact(f"sentinels {tag}", bool((out[2:] == ADAM_SENTINEL).all()) and bool((parts[rows:] == ADAM_SENTINEL).all())
                and _sentinels_ok([G], off, count), "")]
    if kind == "nan":
        vs.append(Exact(f"nan {tag}", bool(torch.isnan(out[0])) and bool(torch.isnan(out[1])) and bool(torch.isnan(norm)), f"{out[:2].tolist()}"))
    elif kind == "inf":
        vs.append(Exact(f"inf {tag}", bool(torch.isinf(out[0])) and float(out[1]) == 0.0 and float(c) == 0.0, f"{out[:2].tolist()}"))
    elif kind == "zero":
        vs.append(Exact(f"zero {tag}", float(out[0]) == 0.0 and float(out[1]) == 1.0 and float(c) == 1.0, f"{out[:2].tolist()}"))
    else:
        vs.append(ElemOnly(compare(f"norm {tag}", out[0:1], norm.reshape(1), norm.reshape(1), 1, F32, "map_f32")))
        vs.append(ElemOnly(compare(f"coef {tag}", out[1:2], c.reshape(1), c.reshape(1), 1, F32, "map_f32")))
        vs.append(Exact(f"coef <= 1 {tag}", float(out[1]) <= 1.0, f"{float(out[1])}"))
    return vs


def check_adam_hp_split(be, dev, count, cut, dc, step0, mode, clip=False, gscale=0.5, seed_no=0) -> List:
    """[cut:] with the step counter, then [:cut] with a scratch counter set to step - 1, each with its slice-relative
    decay_count (optim.Optimizer.split_ops as TrainStep drives it), bit for bit against the single launch"""
    p0, g0, m0, v0, _ = _hp_inputs(count, step0, dev, 1000 + seed_no + count % 1000 + cut)
    st = _stream(dev)
    (b1, b2), eps = ADAM_BETAS, ADAM_EPS
    table = torch.tensor(LR_TABLE, dtype=F32, device=dev)
    coef = torch.tensor([COEF], dtype=F32, device=dev) if clip else None
    kw = dict(weight_decay=WD, decay_mode=mode, clip_coef=coef)
    mk = lambda: [_padded(x, dev, 0) for x in (p0, g0, m0, v0)]
    p, g, m, v = mk()
    step = torch.full((1,), step0, dtype=torch.int64, device=dev)
    be.adam_hp(p, g, m, v, count, table, b1, b2, eps, gscale, step, None, decay_count=dc, **kw)(st)
    P, G, M, V = mk()
    step2 = torch.full((1,), step0, dtype=torch.int64, device=dev)
    tail = torch.zeros(1, dtype=torch.int64, device=dev)
    be.adam_hp(P[cut:], G[cut:], M[cut:], V[cut:], count - cut, table, b1, b2, eps, gscale, step2, None,
               decay_count=min(max(dc - cut, 0), count - cut), **kw)(st)
    torch.sub(step2, 1, out=tail)
    be.adam_hp(P[:cut], G[:cut], M[:cut], V[:cut], cut, table, b1, b2, eps, gscale, tail, None, decay_count=min(dc, cut), **kw)(st)
    _sync(dev)
    tag = f"count {count} cut {cut} dc {dc} step {step0 + 1} mode {mode}"
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    vs = [Exact(f"split {n_} {tag}", bits(a, b), "bit-equal to one launch") for n_, a, b in (("p", P, p), ("m", M, m), ("v", V, v))]
    vs.append(Exact(f"split counters {tag}", int(step2[0]) == step0 + 1 == int(tail[0]) == int(step[0]), f"{int(step2[0])}, {int(tail[0])}"))
    return vs


def hp_case_table(count):
    """(dc, step0, off, shadow, clip, mode index) for one count: every decay_count x step preset, with the slice offset, the
    shadow type, the clipping pointer and the decay mode rotated through them so that each value meets each count"""
    out = []
    i = 0
    for dc in decay_counts(count):
        for s0 in steps0(len(LR_TABLE)):
            out.append((dc, s0, i % 2, SHADOWS[i % 3], (i // 2) % 2 == 1, (i + i // 3) % 3))
            i += 1
    return out


def hp_cross_table():
    """every (off, shadow, clip, mode index) at one count"""
    return [(off, sh, clip, mi) for off in (0, 1) for sh in SHADOWS for clip in (False, True) for mi in range(3)]
