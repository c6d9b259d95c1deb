"""The reference of include/sfk_ema.h in plain torch on the CPU, and the checks tests/test_ema_cpu.py (on the emulated
backend and its mutants) and tests/test_gpu_ema.py (on the kernels) both run.

  ema_rate / ema_weight   d_t and w = (float)(1 - d_t), formed in numpy double from the incremented counter t
  ref_ema                 the fp32 sequence e + w * (p - e): three torch ops, each rounded to fp32 on its own
  ref_lerp64              torch.lerp(e, p, w) in float64
  ema_bound               |fp32 sequence - float64 lerp| <= 1.01 * 2^-24 * (|e'| + 2 w |p - e|), e' the float64 result: the
                          difference and the product carry one rounding each of a term of size w |p - e|, the sum one of
                          size |e'|; 1.01 covers the second-order terms
Inputs (ema_values) have magnitudes in [2^-20, 2^20] with random signs, and every seventh element has p == e exactly: a
nonzero difference is at least 2^-43 and w at least 2^-14, so no intermediate is subnormal and the flush-to-zero settings
of either side cannot enter."""
import numpy as np
import torch

import head_ref64 as H

COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]                # 4099: past one 4096-element tile, with a count % 4 tail
TABLES = {"none": [], "one1": [(1, 0)], "sizes": [(8, 0), (64, 0), (257, 0), (2048, 0)], "offset": [(64, 1)]}   # (n, elements off 16-byte alignment)
DECAYS = [0.0, 0.9, 0.999, 0.9999]
STEPS = [1, 2, 9, 10, 11, 10 ** 6]                           # t, the counter AFTER the launch's increment
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 3)]           # elements p and e start off 16-byte alignment
GUARD = 8                                                    # sentinel elements before and after every array
SENTINEL = -12345.0
SPECIAL_BITS = [0x7fc00000, 0x7f800001, 0x7fc12345, 0x7f800000, -0x00800000, -0x80000000]   # NaNs (three payloads), inf, -inf, -0.0


def ema_rate(decay: float, warmup: bool, t: int) -> float:
    d = np.float64(decay)
    if warmup:
        d = min(d, (np.float64(1.0) + np.float64(t)) / (np.float64(10.0) + np.float64(t)))
    return float(d)


def ema_weight(decay: float, warmup: bool, t: int) -> float:
    return float(np.float32(np.float64(1.0) - np.float64(ema_rate(decay, warmup, t))))


def ref_ema(e: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    assert e.dtype == torch.float32 and p.dtype == torch.float32
    wt = torch.tensor(w, dtype=torch.float32)
    d = p - e
    m = wt * d
    return e + m


def ref_lerp64(e: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    return torch.lerp(e.double(), p.double(), float(w))


def ema_bound(e: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    e64 = ref_lerp64(e, p, w)
    return 1.01 * 2.0 ** -24 * (e64.abs() + 2.0 * w * (p.double() - e.double()).abs())


def ema_values(n: int, seed: int):
    """(p, e) float32 of n elements"""
    g = torch.Generator().manual_seed(seed)

    def draw():
        mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 40.0 - 20.0)
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        return (mag * sign).float().clamp(-2.0 ** 20, 2.0 ** 20)
    p, e = draw(), draw()
    small = p.abs() < 2.0 ** -20
    p[small] = 2.0 ** -20
    small = e.abs() < 2.0 ** -20
    e[small] = 2.0 ** -20
    e[3::7] = p[3::7]
    return p, e


def swap_values(n: int, seed: int):
    """(p, e) as ema_values with NaN (two payloads), inf and -0.0 bit patterns spread in"""
    p, e = ema_values(n, seed)
    pi, ei = p.view(torch.int32), e.view(torch.int32)
    for k, bits in enumerate(SPECIAL_BITS):
        pi[k::13] = bits
        ei[(k + 5)::11] = bits
    return p, e


class Guarded:
    """a float32 array of n elements on `dev`, `off` elements past a 16-byte boundary, with GUARD sentinels on both sides"""

    def __init__(self, values: torch.Tensor, off: int, dev):
        n = values.numel()
        self.n, self.off = n, off
        self.buf = torch.full((off + GUARD + n + GUARD + 4,), SENTINEL, dtype=torch.float32, device=dev)
        lo = GUARD + off                                     # GUARD is a multiple of 4: the view starts `off` past a boundary
        base = self.buf.data_ptr() % 16 // 4
        lo += (4 - base) % 4
        self.lo = lo
        self.view = self.buf[lo:lo + n]
        self.view.copy_(values)
        assert self.view.data_ptr() % 16 == 4 * off

    def guards_intact(self) -> bool:
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all())


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def make_case(dev, count, table, offsets, seed, values=ema_values):
    """(p, e, pairs): Guarded arenas and Guarded (src, dst) pairs of the table spec, with their CPU values"""
    pv, ev = values(count, seed)
    p, e = Guarded(pv, offsets[0], dev), Guarded(ev, offsets[1], dev)
    pairs = []
    for k, (n, off) in enumerate(table):
        sv, dv = values(n, seed * 100 + k + 1)
        pairs.append((Guarded(sv, off, dev), Guarded(dv, off, dev), sv, dv))
    return p, e, pv, ev, pairs


def check_ema_update(be, dev, count, table_name, offsets, decay, warmup, t, seed=0):
    """sfk_ema_update through `be` on `dev` against ref_ema on the CPU, bit for bit; sentinels, sources and the counter"""
    tag = f"ema_update n{count} {table_name} off{offsets} d{decay} wu{int(warmup)} t{t}"
    p, e, pv, ev, pairs = make_case(dev, count, TABLES[table_name], offsets, seed)
    step = torch.tensor([t - 1], dtype=torch.int64, device=dev)
    tab = be.ema_table([(s.view, d.view) for s, d, _, _ in pairs]) if pairs else None
    run = be.ema_update(p.view, e.view, count, tab, decay, warmup, step)
    w = ema_weight(decay, warmup, t)
    vs = []
    for rep in range(2):                                     # a second run from the same state gives the same bits
        e.view.copy_(ev)
        for s, d, sv, dv in pairs:
            d.view.copy_(dv)
        step.fill_(t - 1)
        run(H._stream(dev))
        H._sync(dev)
        vs.append(H.Exact(f"{tag} arena bits run{rep}", torch.equal(_bits(e.view), _bits(ref_ema(ev, pv, w)))))
        for k, (s, d, sv, dv) in enumerate(pairs):
            vs.append(H.Exact(f"{tag} table{k} bits run{rep}", torch.equal(_bits(d.view), _bits(ref_ema(dv, sv, w)))))
        vs.append(H.Exact(f"{tag} counter run{rep}", int(step[0]) == t, f"{int(step[0])}"))
    vs.append(H.Exact(f"{tag} p only read", torch.equal(_bits(p.view), _bits(pv))))
    for k, (s, d, sv, dv) in enumerate(pairs):
        vs.append(H.Exact(f"{tag} src{k} only read", torch.equal(_bits(s.view), _bits(sv))))
    ok = p.guards_intact() and e.guards_intact() and all(s.guards_intact() and d.guards_intact() for s, d, _, _ in pairs)
    vs.append(H.Exact(f"{tag} sentinels", ok))
    return vs


def check_ema_swap(be, dev, count, table_name, offsets, seed=1):
    """sfk_ema_swap: bits exchanged (NaN and inf patterns included), two swaps the identity, counter and sentinels"""
    tag = f"ema_swap n{count} {table_name} off{offsets}"
    p, e, pv, ev, pairs = make_case(dev, count, TABLES[table_name], offsets, seed, values=swap_values)
    tab = be.ema_table([(s.view, d.view) for s, d, _, _ in pairs]) if pairs else None
    run = be.ema_swap(p.view, e.view, count, tab)
    vs = []
    run(H._stream(dev))
    H._sync(dev)
    vs.append(H.Exact(f"{tag} arena exchanged", torch.equal(_bits(p.view), _bits(ev)) and torch.equal(_bits(e.view), _bits(pv))))
    for k, (s, d, sv, dv) in enumerate(pairs):
        vs.append(H.Exact(f"{tag} table{k} exchanged", torch.equal(_bits(s.view), _bits(dv)) and torch.equal(_bits(d.view), _bits(sv))))
    run(H._stream(dev))
    H._sync(dev)
    vs.append(H.Exact(f"{tag} arena twice", torch.equal(_bits(p.view), _bits(pv)) and torch.equal(_bits(e.view), _bits(ev))))
    for k, (s, d, sv, dv) in enumerate(pairs):
        vs.append(H.Exact(f"{tag} table{k} twice", torch.equal(_bits(s.view), _bits(sv)) and torch.equal(_bits(d.view), _bits(dv))))
    ok = p.guards_intact() and e.guards_intact() and all(s.guards_intact() and d.guards_intact() for s, d, _, _ in pairs)
    vs.append(H.Exact(f"{tag} sentinels", ok))
    return vs


def update_cases():
    """(count, table, offsets, decay, warmup, t): every count, table, offset pair, decay, warm-up flag and step of the
    lists above at least once, without their full product"""
    cases = []
    for i, count in enumerate(COUNTS):
        for j, tname in enumerate(TABLES):
            k = i * len(TABLES) + j
            cases.append((count, tname, OFFSETS[0] if k % 2 == 0 else OFFSETS[1 + (k // 2) % 4], DECAYS[k % 4], k % 3 != 0,
                          STEPS[k % 6]))
    for d in DECAYS:                                         # every (decay, warm-up, t) at one unaligned-tail size
        for wu in (False, True):
            for t in STEPS:
                cases.append((1025, "sizes", OFFSETS[0], d, wu, t))
    for off in OFFSETS[1:]:
        cases.append((4099, "offset", off, 0.999, True, 9))
    return cases


def swap_cases():
    cases = [(c, tname, OFFSETS[0]) for c in COUNTS for tname in TABLES]
    return cases + [(c, "sizes", off) for c in (5, 4099) for off in OFFSETS[1:]]


# ------------------------------------------------------------------ the whole route
def stat_pairs_cpu(eng):
    return [(a.detach().cpu().clone(), b.detach().cpu().clone()) for a, b in eng.ema_stat_pairs()]


def recursion(avg, snapshots, decay, warmup):
    """the reference recursion: avg (a list of CPU tensors) through ref_ema over the per-step snapshots (lists of CPU
    tensors taken after each step), with t = 1, 2, ..."""
    for t, snap in enumerate(snapshots, start=1):
        w = ema_weight(decay, warmup, t)
        avg = [ref_ema(a, s, w) for a, s in zip(avg, snap)]
    return avg


def live_snapshot(eng):
    return [eng.P.data.detach().cpu().clone()] + [a for a, _ in stat_pairs_cpu(eng)]


def ema_snapshot(eng):
    return [eng.ema_P.detach().cpu().clone()] + [b for _, b in stat_pairs_cpu(eng)]


def check_route(eng, step_fn, steps, decay, warmup):
    """runs step_fn() `steps` times, snapshots P / rm / rv after each, and compares ema_P / the averaged statistics with the
    recursion over THIS run's snapshots, bit for bit.  The average must exist already (TrainStep built)."""
    avg0, snaps = ema_snapshot(eng), []
    t0 = int(eng.ema_step[0])
    assert t0 == 0, t0
    for _ in range(steps):
        step_fn()
        snaps.append(live_snapshot(eng))
    want, got = recursion(avg0, snaps, decay, warmup), ema_snapshot(eng)
    vs = [H.Exact(f"route tensor{k} bits", torch.equal(_bits(a), _bits(b))) for k, (a, b) in enumerate(zip(got, want))]
    vs.append(H.Exact("route counter", int(eng.ema_step[0]) == steps))
    vs.append(H.Exact("route average moved", not torch.equal(got[0], avg0[0])))
    return vs
