"""TEST INFRASTRUCTURE for include/sfk_groups.h: the segment tables and the checks that hold one grouped launch of a backend
(HipBackend on the GPU, EmuGroupsBackend and its mutants on the CPU) to the header's contract, bit for bit, against the _hp
entry points of a reference backend (HipBackend itself on the GPU, the unmutated EmuOptimBackend on the CPU), and element by
element against float64 (tests/optim_ref64.py) under the project's existing bounds."""
from __future__ import annotations

from typing import List

import torch

import optim_ref64 as O
from head_ref64 import (ADAM_BETAS, ADAM_EPS, ADAM_PAD, ADAM_SENTINEL, BF16, F32, Exact, _stream, _sync, adam_inputs, compare_p)
from ref64 import F64, compare

NGROUPS = 3
LR_ROWS = [[0.05, 0.03, 0.02, 0.01], [0.005, 0.003, 0.002, 0.001], [0.02, 0.04, 0.01, 0.03]]      # three rows that differ
WDS = [0.5, 0.05, 0.25]
EDGES = (0, 1, 3, 4, 5, 1023, 1024, 1025)


def seg_all(count):
    """one all-covering group: must equal one _hp launch on the whole arena"""
    return [(0, count, 0, 1)]


def seg_bounds(count):
    """boundaries at 0, 1, 3, 4, 5, 1023..1025, count-1 and count; the ranges between them rotate through the groups and the
    decay flag, every fourth is frozen; the first and the last range are covered"""
    cuts = sorted({c for c in EDGES + (count - 1, count) if 0 <= c <= count})
    rng = list(zip(cuts[:-1], cuts[1:]))
    out = []
    for i, (b, e) in enumerate(rng):
        if i % 4 == 2 and 0 < i < len(rng) - 1:
            continue
        out.append((b, e, i % NGROUPS, i % 2))
    return out


def seg_alternating(count):
    """covered and frozen runs of 1..7 elements in turn"""
    out, pos, k = [], 0, 0
    while pos < count:
        n = min(1 + (k * 3) % 7, count - pos)
        if k % 2 == 0:
            out.append((pos, pos + n, (k // 2) % NGROUPS, (k // 2) % 2))
        pos += n
        k += 1
    return out


def seg_many(count, nseg=1000):
    """about nseg segments over the three groups with unaligned bounds and gaps of a few elements; the last ends at count"""
    stride = max(count // nseg, 2)
    out = []
    for k in range(nseg):
        b = k * stride + (k % 5 if stride > 8 else 0)
        e = (k + 1) * stride - ((1 + k % 3) if stride > 8 else 1)
        if b >= count:
            break
        e = min(e, count)
        if e > b:
            out.append((b, e, k % NGROUPS, (k // 3) % 2))
    b, _, grp, dec = out[-1]
    out[-1] = (b, count, grp, dec)
    return out


def tables_for(count):
    t = {"all": seg_all(count), "empty": [], "bounds": seg_bounds(count), "alternating": seg_alternating(count)}
    if count >= 4099:
        t["many"] = seg_many(count)
    return t


def _bits(a, b) -> bool:
    ia = a.view(torch.int16 if a.element_size() == 2 else (torch.int32 if a.element_size() == 4 else torch.int64))
    ib = b.view(ia.dtype)
    return torch.equal(ia, ib)


def _same_or_nan(a, b) -> bool:
    return _bits(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)))


def _inputs(count, step0, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p, g, m, v, _ = adam_inputs(count, step0, gen)
    return p, g, m, v


def _rows(dev, ngroups):
    return (torch.tensor(LR_ROWS[:ngroups], dtype=F32, device=dev).contiguous(), WDS[:ngroups])


def check_update_groups(be, ref, dev, kernel, count, segments, step0=1, off=0, shadow_dtype=None, clip=False, mode="l2",
                        gscale=0.5, nesterov=False, momentum=O.SGD_MOM, ngroups=NGROUPS, ref64=False, tag="") -> List:
    """one sfk_adam_groups / sfk_sgd_groups launch of `be` against the contract: `ref`'s adam_hp / sgd_hp on every segment's
    slice with a cloned step counter; uncovered elements and the sentinels around the arena keep their bits; the step is
    incremented once.  ref64: every covered element also against optim_ref64's float64 restatement, existing bounds."""
    adam = kernel == "adam"
    p0, g0, m0, v0 = _inputs(count, step0, dev, 1300 + count % 1000 + step0 + len(segments))
    st = _stream(dev)
    rows, wds = _rows(dev, ngroups)
    coef = torch.tensor([O.COEF], dtype=F32, device=dev) if clip else None
    (b1, b2), eps = ADAM_BETAS, ADAM_EPS
    use_buf = adam or momentum != 0

    def fresh():
        bufs = [O._padded(x, dev, off) for x in ((p0, g0, m0, v0) if adam else (p0, g0, m0))]
        sh = None if shadow_dtype is None else torch.full((off + count + ADAM_PAD,), ADAM_SENTINEL, dtype=shadow_dtype, device=dev)
        return bufs, sh, torch.full((1,), step0, dtype=torch.int64, device=dev)

    (A, SH, step), (R, RSH, rstep) = fresh(), fresh()
    table = be.group_table(segments, wds, count, dev)
    sl = lambda x: None if x is None else x[off:]
    if adam:
        be.adam_groups(sl(A[0]), sl(A[1]), sl(A[2]), sl(A[3]), count, table, rows, b1, b2, eps, gscale, step, sl(SH),
                       decay_mode=mode, clip_coef=coef)(st)
    else:
        be.sgd_groups(sl(A[0]), sl(A[1]), sl(A[2]), count, table, rows, momentum, O.SGD_DAMP, nesterov, gscale, step, sl(SH),
                      decay_mode=mode, clip_coef=coef)(st)
    for b, e, grp, dec in segments:
        s_ = torch.full((1,), step0, dtype=torch.int64, device=dev)
        cut = lambda x: None if x is None else x[off + b: off + e]
        kw = dict(weight_decay=wds[grp], decay_mode=mode, decay_count=e - b if dec else 0, clip_coef=coef)
        if adam:
            ref.adam_hp(cut(R[0]), cut(R[1]), cut(R[2]), cut(R[3]), e - b, rows[grp], b1, b2, eps, gscale, s_, cut(RSH), **kw)(st)
        else:
            ref.sgd_hp(cut(R[0]), cut(R[1]), cut(R[2]), e - b, rows[grp], momentum, O.SGD_DAMP, nesterov, gscale, s_, cut(RSH),
                       **kw)(st)
    _sync(dev)
    tag = f"{kernel}_groups {tag} count {count} segs {len(segments)} step {step0 + 1} off {off} shadow {shadow_dtype} clip {clip} mode {mode}"
    names = ("p", "g", "m", "v") if adam else ("p", "g", "buf")
    vs = [Exact(f"step {tag}", int(step[0]) == step0 + 1, f"{int(step[0])}")]
    for n_, a, r in zip(names, A, R):
        vs.append(Exact(f"{n_} bit-equal to the _hp launches, sentinels and frozen elements included {tag}", _bits(a, r), ""))
    if SH is not None:
        vs.append(Exact(f"shadow bit-equal {tag}", _bits(SH, RSH), str(shadow_dtype)))
    # the reference side itself left what no segment covers alone (so "equal to it" means "frozen")
    keep = torch.ones(count, dtype=torch.bool, device=dev)
    for b, e, _, _ in segments:
        keep[b:e] = False
    for n_, a, x0 in zip(names, A, (p0, g0, m0, v0)):
        vs.append(Exact(f"{n_} frozen elements keep their bits {tag}", _bits(a[off: off + count][keep], x0[keep]), f"{int(keep.sum())}"))
    vs.append(Exact(f"sentinels {tag}", O._sentinels_ok(A + ([SH] if SH is not None else []), off, count), ""))
    if SH is not None:
        vs.append(Exact(f"shadow frozen elements untouched {tag}", bool((SH[off: off + count][keep].float() == ADAM_SENTINEL).all()), ""))
    if int((g0[~keep] != 0).sum()) >= 32:                # (a few elements may all sit in adam_inputs' block of p = g = 0, or absorb lr * g)
        vs.append(Exact(f"something moved {tag}", not _bits(A[0][off: off + count], p0), ""))
    if not use_buf:
        vs.append(Exact(f"buf untouched {tag}", _bits(A[2][off: off + count], m0), ""))
    if ref64:
        table_rows = rows.cpu().tolist()
        for b, e, grp, dec in segments:
            dc = e - b if dec else 0
            cutp = lambda x: x[off + b: off + e]
            if adam:
                r = O.adam_hp_ref(p0[b:e], g0[b:e], m0[b:e], v0[b:e], step0 + 1, table_rows[grp], b1, b2, eps, gscale,
                                  wds[grp], mode, dc, O.COEF if clip else None)
                vs += [compare(f"m [{b},{e}) {tag}", cutp(A[2]), r["m"], r["a_m"], 2, F32, "map_f32"),
                       compare(f"v [{b},{e}) {tag}", cutp(A[3]), r["v"], r["a_v"], 2, F32, "map_f32"),
                       compare_p(f"p [{b},{e}) {tag}", cutp(A[0]), r)]
            else:
                r = O.sgd_hp_ref(p0[b:e], g0[b:e], m0[b:e], step0 + 1, table_rows[grp], momentum, O.SGD_DAMP, nesterov, gscale,
                                 wds[grp], mode, dc, O.COEF if clip else None)
                vs.append(compare(f"p [{b},{e}) {tag}", cutp(A[0]), r["p"], r["a_p"], 4, F32, "map_f32"))
                if momentum != 0:
                    vs.append(compare(f"buf [{b},{e}) {tag}", cutp(A[2]), r["buf"], r["a_buf"], 3, F32, "map_f32"))
    return vs


def check_norm_groups(be, ref, dev, count, segments, kind="randn", off=0, gscale=0.5, ngroups=NGROUPS, tag="") -> List:
    """sfk_grad_norm_groups of `be` against `ref`'s grad_norm on a copy with the uncovered elements zeroed: out and partials
    bit for bit, and the same bits on a second run.  kind 'nan_frozen' / 'inf_frozen' put the value into an uncovered element
    (it must not show), 'nan' / 'inf' into a covered one."""
    g0 = O.norm_inputs(count, dev, "randn")
    keep = torch.zeros(count, dtype=torch.bool, device=dev)
    for b, e, _, _ in segments:
        keep[b:e] = True
    val = float(kind.split("_")[0]) if kind != "randn" else None
    placed = True
    if val is not None:
        idx = torch.nonzero(~keep if kind.endswith("_frozen") else keep).reshape(-1)
        placed = idx.numel() > 0
        if placed:
            g0[idx[idx.numel() // 2]] = val
    st = _stream(dev)
    max_norm = 0.25
    G = O._padded(g0, dev, off)
    Z = O._padded(torch.where(keep, g0, torch.zeros_like(g0)), dev, off)
    rows = ref.grad_norm_parts(count)
    table = be.group_table(segments, WDS[:ngroups], count, dev)
    outs = []
    for grouped in (True, True, False):                  # the grouped launch twice, then the plain norm of the zeroed copy
        parts = torch.full((rows + 2,), ADAM_SENTINEL, dtype=F64, device=dev)
        out = torch.full((4,), ADAM_SENTINEL, dtype=F32, device=dev)
        if grouped:
            be.grad_norm_groups(G[off:], count, table, gscale, max_norm, parts, out)(st)
        else:
            ref.grad_norm(Z[off:], count, gscale, max_norm, parts, out)(st)
        _sync(dev)
        outs.append((out, parts))
    (o1, p1), (o2, p2), (oz, pz) = outs
    tag = f"grad_norm_groups {tag} count {count} segs {len(segments)} {kind} off {off}"
    vs = [Exact(f"out bit-equal to grad_norm on the zeroed copy {tag}", _same_or_nan(o1, oz), f"{o1[:2].tolist()} {oz[:2].tolist()}"),
          Exact(f"partials bit-equal {tag}", _same_or_nan(p1, pz), ""),
          Exact(f"second run bit-equal {tag}", _same_or_nan(o1, o2) and _same_or_nan(p1, p2), ""),
          Exact(f"g untouched, sentinels {tag}", _same_or_nan(G[off: off + count], g0) and O._sentinels_ok([G], off, count), "")]
    if placed and kind.endswith("_frozen"):
        vs.append(Exact(f"a frozen {kind} does not show {tag}", bool(torch.isfinite(o1[:2]).all()), f"{o1[:2].tolist()}"))
    elif placed and kind == "nan":
        vs.append(Exact(f"a covered nan shows {tag}", bool(torch.isnan(o1[0])), f"{o1[:2].tolist()}"))
    elif placed and kind == "inf":
        vs.append(Exact(f"a covered inf shows {tag}", bool(torch.isinf(o1[0])) and float(o1[1]) == 0.0, f"{o1[:2].tolist()}"))
    elif segments:
        vs.append(Exact(f"norm > 0 {tag}", float(o1[0]) > 0, f"{o1[:2].tolist()}"))
    return vs


def update_case_table(count):
    """(table name, segments, kernel, off, shadow, clip, mode, nesterov, momentum) for one count: every segment table with each
    kernel, the offset, shadow type, clipping pointer, decay mode and SGD flavour rotated through them"""
    out, i = [], 0
    for name, segs in tables_for(count).items():
        for kernel in ("adam", "sgd"):
            modes = O.MODES if kernel == "adam" else O.MODES[:2]
            out.append((name, segs, kernel, i % 2, O.SHADOWS[i % 3], (i // 2) % 2 == 1, modes[(i + i // 3) % len(modes)],
                        i % 4 == 1, 0.0 if (kernel == "sgd" and i % 5 == 3) else O.SGD_MOM))
            i += 1
    return out
