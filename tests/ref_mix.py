"""TEST INFRASTRUCTURE for include/sfk_mix.h: the mix as a plain torch expression, the soft-target loss restated in float64
with its |terms| companion, the case tables, and the checks that run one case on a backend (HipBackend on the GPU,
EmuMixBackend and its mutants on the CPU) and return the verdicts.  tests/test_gpu_mix.py and tests/test_mix_cpu.py import
the checks from here, so a mutant is refused by exactly what the GPU file runs.

ref_mix is `lam * x + (1 - lam) * x[partner]` with the box pasted, in fp32 (torch on the CPU rounds each op on its own),
then `.to(dtype)`; ref_softmax_ce_mix follows tests/head_ref64.py::softmax_ce and is held to ref64.elem_bound / compare as
they stand, with the `extra` term that function derives for the normaliser.  The loss's reduction length is n without
smoothing (n row losses) and n * K with it (the smoothing term sums every logit of every row)."""
from __future__ import annotations

import math
from typing import List

import torch

import head_ref64 as H
from ref64 import EPS32, F64, compare, elem_bound

F32, BF16 = torch.float32, torch.bfloat16


# ----------------------------------------------------------------------------- rows
def identity_rows(n: int) -> torch.Tensor:
    r = torch.zeros(n, 8, dtype=F32)
    r[:, 0] = torch.arange(n, dtype=F32)
    r[:, 1] = 1.0
    r[:, 6] = 1.0
    return r


def partners(rows: torch.Tensor) -> torch.Tensor:
    """the partner of every row as the kernels read it: out of [0, n) or not mutual -> the row itself"""
    n = rows.shape[0]
    pf = rows[:, 0].double()
    ok = (pf >= 0) & (pf < n)
    p = torch.where(ok, pf, torch.arange(n, dtype=F64)).long()
    mutual = ok & (p[p] == torch.arange(n)) & ok[p]
    return torch.where(mutual, p, torch.arange(n))


def boxes(rows: torch.Tensor, h: int, w: int):
    """[(y0, x0, y1, x1)] clamped to the frame, None for an empty box"""
    out = []
    for r in rows.tolist():
        y0, x0, y1, x1 = (int(min(max(v, 0), lim)) for v, lim in zip(r[2:6], (h, w, h, w)))
        out.append((y0, x0, y1, x1) if y1 > y0 and x1 > x0 else None)
    return out


# ----------------------------------------------------------------------------- the mix
def ref_mix(x: torch.Tensor, rows: torch.Tensor, c_off: int = 0, c: int = None) -> torch.Tensor:
    """x (N, T, C, H, W) f32 | bf16 -> a new tensor with channels c_off .. c_off + c - 1 mixed as sfk_clip_mix mixes them"""
    rows = rows.detach().cpu().to(F32)
    n, _, ch, h, w = x.shape
    c = ch - c_off if c is None else c
    out = x.clone()
    src = x[:, :, c_off:c_off + c].to(F32)
    p = partners(rows)
    lam = rows[:, 1].view(n, 1, 1, 1, 1).to(src.device)
    other = src[p.to(src.device)]
    mixed = torch.where(lam == 1, src, lam * src + (1 - lam) * other)      # lam == 1 outside the box: the value itself
    for i, b in enumerate(boxes(rows, h, w)):
        if int(p[i]) == i:
            mixed[i] = src[i]                                              # identity by the guard, or a self pair
        elif b is not None:
            y0, x0, y1, x1 = b
            mixed[i, :, :, y0:y1, x0:x1] = other[i, :, :, y0:y1, x0:x1]
    out[:, :, c_off:c_off + c] = mixed.to(x.dtype)
    return out


# pair specs (row of the lower member, row of the upper member), each (lam, box | None) on an h x w frame
def pair_specs(h: int, w: int):
    e = None
    return [
        ((0.3, e), (0.3, e)), ((0.0, e), (0.0, e)), ((0.5, e), (0.5, e)),
        ((1.0, e), (1.0, e)),                                             # a both-identity pair
        ((1.0, (0, 0, h, w)), (1.0, (0, 0, h, w))),                       # the full frame
        ((1.0, (3, 5, 4, 6)), (1.0, (3, 5, 4, 6))),                       # one pixel
        ((1.0, (0, 2, 4, 9)), (1.0, (0, 2, 4, 9))),                       # touching the top edge
        ((1.0, (h - 3, 1, h, w - 2)), (1.0, (h - 3, 1, h, w - 2))),       # ... the bottom edge
        ((1.0, (2, 0, 7, 5)), (1.0, (2, 0, 7, 5))),                       # ... the left edge
        ((1.0, (1, w - 6, 6, w)), (1.0, (1, w - 6, 6, w))),               # ... the right edge
        ((1.0, (2, 3, h - 1, w - 5)), (1.0, (2, 3, h - 1, w - 5))),       # x0, x1 no multiples of 8
        ((0.3, (1, 2, 5, 11)), (1.0, (4, 9, 9, 14))),                     # the two members carry different rows
        ((1.0, e), (0.3, e)),                                             # one member identity, the other blended
        ((1.0, (0, 8, 5, 16)), (0.5, e)),                                 # a whole aligned unit pasted / a blend
    ]


def mix_row_sets(n: int, h: int, w: int) -> List[torch.Tensor]:
    """row tables for n clips that together cover every pair spec; pairing is the flip (the middle clip of an odd batch is a
    self pair), and for n = 6 every other table pairs 0-3, 1-5, 2-4 instead"""
    specs = pair_specs(h, w)
    if n < 2:
        return [identity_rows(n)]
    npairs, sets = n // 2, []
    for v in range(math.ceil(len(specs) / npairs)):
        rows = identity_rows(n)
        pairing = [(i, n - 1 - i) for i in range(npairs)]
        if n == 6 and v % 2 == 1:
            pairing = [(0, 3), (1, 5), (2, 4)]
        for q, (a, b) in enumerate(pairing):
            ra, rb = specs[(v * npairs + q) % len(specs)]
            for i, j, (lam, box) in ((a, b, ra), (b, a, rb)):
                rows[i, 0], rows[i, 1] = float(j), lam
                if box is not None:
                    rows[i, 2:6] = torch.tensor(box, dtype=F32)
                rows[i, 6] = lam if box is None else 1.0 - (box[2] - box[0]) * (box[3] - box[1]) / float(h * w)
        sets.append(rows)
    return sets


MIX_SIZES = [(17, 19), (32, 32)]
# name -> (channels of the clip, c_off, mixed channels, stray elements between two clips)
MIX_LAYOUTS = {"7ch": (7, 0, 7, 0), "21ch": (21, 0, 21, 0), "5of7_gap5": (7, 2, 5, 5)}
MIX_N = [1, 2, 5, 6]


def _stream(dev):
    return torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else 0


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def on_device(x: torch.Tensor, dev, gap: int = 0, dtype=F32, guard: int = 64):
    """x in a pattern-filled buffer on `dev` with `gap` elements between two clips and `guard` after the last: (view, buffer)"""
    n, per = x.shape[0], x[0].numel()
    buf = torch.arange(n * (per + gap) + guard, dtype=F32).mul_(0.37).sub_(11).to(dtype).to(dev)
    view = buf[:n * (per + gap)].view(n, per + gap)[:, :per].view(x.shape)
    view.copy_(x.to(dtype))
    return view, buf


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def mix_input(n, t, ch, h, w, dtype, seed=0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * h + w)
    x = torch.randn(n, t, ch, h, w, generator=g) * 2.0
    x[:, :, :, 1, :3] = 0.0                                   # zeros of both signs among the values
    x[:, :, :, 2, :3] = -0.0
    return x.to(dtype)


def check_clip_mix(be, dev, h: int, w: int, layout: str, n: int, dtype, t: int = 2) -> List:
    """every row table of mix_row_sets on one geometry: the clip's bits against ref_mix, everything outside the mixed channels,
    identity pairs and self clips unchanged, and a second run from the same input"""
    ch, c_off, c, gap = MIX_LAYOUTS[layout]
    x = mix_input(n, t, ch, h, w, dtype)
    vs, tag = [], f"{h}x{w}-{layout}-n{n}-{str(dtype)[6:]}"
    for v, rows in enumerate(mix_row_sets(n, h, w)):
        want = ref_mix(x, rows, c_off, c)
        runs = []
        for _ in range(2):
            view, buf = on_device(x, dev, gap, dtype)
            before = buf.clone()
            be.clip_mix(view, rows.to(dev), c_off, c)(_stream(dev))
            _sync(dev)
            runs.append((view.cpu(), buf.cpu(), before.cpu()))
        got, buf, before = runs[0]
        bad = int((_bits(got) != _bits(want)).sum())
        vs.append(H.Exact(f"clip_mix bits {tag} set {v}", bad == 0, f"{bad} elements differ"))
        inside = torch.zeros(buf.shape, dtype=torch.bool)
        inside[:n * (x[0].numel() + gap)].view(n, -1)[:, :x[0].numel()].view(x.shape)[:, :, c_off:c_off + c] = True
        changed = _bits(buf) != _bits(before)
        vs.append(H.Exact(f"clip_mix outside {tag} set {v}", not bool((changed & ~inside).any()),
                          f"{int((changed & ~inside).sum())} elements outside the mixed channels changed"))
        p = partners(rows)
        still = [i for i in range(n) if int(p[i]) == i or (bool((rows[i, 1:6] == identity_rows(1)[0, 1:6]).all())
                                                           and bool((rows[int(p[i]), 1:6] == identity_rows(1)[0, 1:6]).all()))]
        same = all(bool((_bits(got[i]) == _bits(x[i])).all()) for i in still)
        vs.append(H.Exact(f"clip_mix identity / self clips {tag} set {v}", same, f"clips {still}"))
        vs.append(H.Exact(f"clip_mix second run {tag} set {v}", bool((_bits(runs[1][1]) == _bits(buf)).all())))
    return vs


# ----------------------------------------------------------------------------- the loss
def ref_softmax_ce_mix(logits: torch.Tensor, labels: torch.Tensor, rows, eps: float, gscale: float):
    """float64 from the float32 logits -> dict(dl, a (the normaliser's extra term folded in, as head_ref64.softmax_ce folds
    it), loss, a_loss, correct).  rows None: identity.  A label whose weight is exactly 0 contributes nothing to the loss."""
    x = logits.to(F64)
    n, k = x.shape
    dev = x.device
    gs, e = H.f32(gscale), H.f32(eps)
    ar = torch.arange(n, device=dev)
    if rows is None:
        p2, w = ar, torch.ones(n, dtype=F64, device=dev)
    else:
        r = rows.detach().cpu().to(F32)
        pf = r[:, 0].double()
        p2 = torch.where((pf >= 0) & (pf < n), pf, torch.arange(n, dtype=F64)).long().to(dev)      # out of range means self
        w = r[:, 6].double().to(dev)
    y1, y2 = labels.long(), labels.long()[p2]
    mx = x.max(1, keepdim=True).values
    d = x - mx
    ex = d.exp()
    s = ex.sum(1, keepdim=True)
    p = ex / s
    t = torch.zeros_like(p)
    t[ar, y1] += w
    t[ar, y2] += 1.0 - w
    t = (1.0 - e) * t + e / k
    dl = (p - t) / n * gs
    a = (p + t) / n * abs(gs)
    dist = torch.where(torch.isinf(d), torch.zeros_like(d), -d)
    extra = 2.0 * EPS32 * (dist * p + p * (p * dist).sum(1, keepdim=True)) / n * abs(gs)
    a_eff = a + extra / (EPS32 * (16.0 + 2.0 * math.sqrt(k)))
    lse, alse = (s.log() + mx).view(n), (s.log().abs() + mx.abs()).view(n)
    z1, z2 = x[ar, y1], x[ar, y2]
    zero = torch.zeros(n, dtype=F64, device=dev)
    l1, a1 = torch.where(w != 0, w * (lse - z1), zero), torch.where(w != 0, w * (alse + z1.abs()), zero)
    l2, a2 = torch.where(w != 1, (1 - w) * (lse - z2), zero), torch.where(w != 1, (1 - w) * (alse + z2.abs()), zero)
    loss_n, a_n = (1.0 - e) * (l1 + l2), (1.0 - e) * (a1 + a2)
    if e > 0:
        loss_n = loss_n + (e / k) * (k * lse - x.sum(1))
        a_n = a_n + (e / k) * (k * alse + x.abs().sum(1))
    idx = torch.arange(k, device=dev).expand(n, k)
    first = torch.where(x == mx, idx, torch.full_like(idx, k)).min(1).values
    judged = torch.where(w >= 0.5, y1, y2)
    return dict(dl=dl, a=a_eff, loss=loss_n.sum() / n, a_loss=a_n.sum() / n, correct=int((first == judged).sum()))


CE_MIX_K = [1, 7, 249, 257, 1000]
CE_MIX_N = [1, 5]
CE_MIX_EPS = [0.0, 0.1]
CE_MIX_KINDS = ["sd1", "sd40", "shift3e4", "equal", "neginf"]
CE_MIX_CASES = [(k, n, e, s) for k in CE_MIX_K for n in CE_MIX_N for e in CE_MIX_EPS for s in CE_MIX_KINDS
                if not (s == "neginf" and k < 2)]
CE_MIX_W = [1.0, 0.5, 0.3, 0.0]


def ce_mix_row_sets(n: int) -> List[torch.Tensor]:
    """identity, then weights {1, 0.5, 0.3, 0} rotated over the rows with partners other (the flip) and self"""
    sets = [identity_rows(n)]
    for v in range(4):
        rows = identity_rows(n)
        if v % 2 == 0:
            rows[:, 0] = torch.arange(n - 1, -1, -1, dtype=F32)
        rows[:, 6] = torch.tensor([CE_MIX_W[(i + v) % 4] for i in range(n)])
        sets.append(rows)
    return sets


def _loss_verdict(name, got, ref, a, pre, kred):
    if not math.isfinite(float(ref)):
        return H.Exact(name, float(got[0]) == float(ref), f"{float(got[0])} want {float(ref)}")
    return H.ElemOnly(compare(name, got, ref + pre, a + abs(pre), kred, F32, "sum_f32"))


def _run_ce_mix(be, dev, x, labels, rows, eps, gscale, tag) -> List:
    n, k = x.shape
    st = _stream(dev)
    x, labels = x.to(dev), labels.to(dev)
    rd = None if rows is None else rows.to(dev)
    pre_l, pre_s, pre_c = 1.5, -2.25, 7
    dl = torch.full((n, k), float("nan"), device=dev)
    lo, ls = torch.full((1,), pre_l, device=dev), torch.full((1,), pre_s, device=dev)
    co = torch.full((1,), pre_c, dtype=torch.int32, device=dev)
    be.softmax_ce_mix(x, labels, rd, eps, n, k, gscale, dl, lo, ls, co)(st)
    ls2, co2 = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    be.softmax_ce_mix(x, labels, rd, eps, n, k, gscale, None, None, ls2, co2)(st)
    _sync(dev)
    ref = ref_softmax_ce_mix(x, labels, rows, eps, gscale)
    vs = [compare(f"dlogits {tag}", dl, ref["dl"], ref["a"], k, F32, "map_f32")]
    bnd = elem_bound(ref["dl"], ref["a"], k, F32)
    rs, rb = dl.double().sum(1).abs(), bnd.sum(1)
    ok = bool((torch.nan_to_num(rs, nan=float("inf")) <= rb).all())
    vs.append(H.Exact(f"dlogits rows sum to 0 {tag}", ok, f"worst {float(torch.nan_to_num(rs / rb, nan=float('inf')).max()):.3g} of the bound"))
    kred = n * k if eps > 0 else n
    for name, got, pre in (("loss_out", lo, pre_l), ("loss_sum", ls, pre_s), ("loss_sum eval", ls2, 0.0)):
        vs.append(_loss_verdict(f"{name} {tag}", got, ref["loss"], ref["a_loss"], pre, kred))
    vs.append(H.Exact(f"correct {tag}", int(co[0]) == pre_c + ref["correct"], f"{int(co[0])} want {pre_c + ref['correct']}"))
    vs.append(H.Exact(f"correct eval {tag}", int(co2[0]) == ref["correct"], f"{int(co2[0])} want {ref['correct']}"))
    return vs, dl, co


def check_ce_mix(be, dev, case, gscale: float = 0.37, seed_no: int = 0) -> List:
    """one (k, n, eps, family) case over ce_mix_row_sets(n), one table with y1 == y2 in a row whose partner is another row,
    and -- with eps == 0 -- dlogits and correct of the identity table and of rows = NULL against sfk_softmax_ce, bit for bit"""
    k, n, eps, kind = case
    gen = torch.Generator().manual_seed(300 + seed_no + 7 * k + n)
    x, labels = H.ce_logits(k, n, kind, gen)
    tag = f"k{k}-n{n}-eps{eps}-{kind}"
    vs = []
    for v, rows in enumerate(ce_mix_row_sets(n)):
        lab = labels.clone()
        if v == 3 and n > 1:
            lab[n - 1] = lab[0]                       # y1 == y2 in rows 0 and n - 1 (flip partners)
        got, dl, co = _run_ce_mix(be, dev, x, lab, rows, eps, gscale, f"{tag} set {v}")
        vs += got
    if eps == 0:
        st = _stream(dev)
        xd, ld = x.to(dev), labels.to(dev)
        dl0 = torch.full((n, k), float("nan"), device=dev)
        lo0, c0 = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        be.softmax_ce(xd, ld, n, k, gscale, dl0, lo0, None, c0)(st)
        for name, rows in (("identity rows", identity_rows(n).to(dev)), ("rows NULL", None)):
            dl1 = torch.full((n, k), float("nan"), device=dev)
            lo1, c1 = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            be.softmax_ce_mix(xd, ld, rows, 0.0, n, k, gscale, dl1, lo1, None, c1)(st)
            _sync(dev)
            same = bool((dl1.view(torch.int32) == dl0.view(torch.int32)).all()) and int(c1[0]) == int(c0[0])
            vs.append(H.Exact(f"bits of sfk_softmax_ce, {name} {tag}", same))
    return vs


def check_ce_mix_correct(be, dev) -> List:
    """`correct` on head_ref64's tie rows (the first of two equal maxima counts): the judged label is y1 at weight >= 0.5
    -- 0.5 itself included -- and y2 below; partners 0-1, 2-3 and 4 with itself"""
    x, labels = H.ce_tie_logits(torch.Generator().manual_seed(11))
    n, k = x.shape
    vs = []
    for name, ws in (("w 0.5", [0.5] * 5), ("w mixed", [0.3, 0.5, 0.3, 1.0, 0.0]), ("w 0", [0.0] * 5), ("w 0.7", [0.7] * 5)):
        rows = identity_rows(n)
        rows[:, 0] = torch.tensor([1.0, 0.0, 3.0, 2.0, 4.0])
        rows[:, 6] = torch.tensor(ws)
        for eps in (0.0, 0.1):
            got, _, _ = _run_ce_mix(be, dev, x, labels, rows, eps, 1.0, f"ties {name} eps{eps}")
            vs += got
    return vs
