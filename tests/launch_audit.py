"""TEST INFRASTRUCTURE: record the conv / stem / BatchNorm launches a training plan binds, as geometry-only signatures, and
replay each one on fresh seeded buffers against the float64 restatement (tests/ref64.py).

  * ``Recorder(backend)`` forwards every attribute of the backend it wraps; for the methods in AUDITED it stores a
    signature (dtypes, extents, ld / c_off, strides, 256-byte base alignment, which optional operands are bound, byte
    overlaps between operands, and for a conv the family the backend reports) and then delegates.  A signature holds no
    tensor, so the plan can be freed before anything is replayed.
  * ``replay(sig, backend)`` allocates the recorded geometry, fills it (seeded), runs the launch once and returns one
    Verdict per output (the tolerance policy of ref64.compare) plus an ``untouched`` check: every byte of every buffer
    outside the written region -- other channels of a wider pixel record, stem-layout padding, partial rows past the ones
    reported, a guard after every buffer -- is unchanged.
A method or operand variant this file does not restate raises NotImplementedError: nothing is skipped silently.
Adding a method is one entry in AUDITED plus one restatement in _REFS."""
from __future__ import annotations

import dataclasses
import inspect
import math
from typing import Dict

import torch

import ref64
from ref64 import F64
from video_classification_amd._lib import (BnBwdFuse, ConvEpilogue, ConvPass, FMap, StemSrc, WgradPass, stem_kp)

AUDITED = ("conv_igemm", "conv_wgrad", "conv_pw_dual", "stem_conv_fwd", "stem_conv_wgrad", "stem2d_fwd", "stem2d_wgrad",
           "bn_stats", "bn_bwd_reduce", "bn_bwd_finalize", "bn_maxpool_fwd", "bn_maxpool_bwd_reduce", "bn_maxpool_bwd_apply")
_DC = {c.__name__: c for c in (ConvPass, WgradPass, StemSrc, ConvEpilogue, BnBwdFuse)}
_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
_DTN = {v: k for k, v in _DT.items()}
GUARD = 1024          # bytes after every replayed buffer that no launch may touch


# ============================================================================= recording
def _leaves(v, path, out):
    """(path, object) of every tensor / FMap inside an argument, in a fixed order"""
    if isinstance(v, FMap) or torch.is_tensor(v):
        out.append((path, v))
    elif dataclasses.is_dataclass(v):
        for f in dataclasses.fields(v):
            _leaves(getattr(v, f.name), path + (f.name,), out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _leaves(x, path + (i,), out)


def _span(v):
    """(storage base, first byte, one past the last byte) an operand covers"""
    if isinstance(v, FMap):
        lo = v.buf.data_ptr()
        return v.buf.untyped_storage().data_ptr(), lo, lo + v.pixels * v.ld * v.buf.element_size()
    if v.numel() == 0:
        return v.untyped_storage().data_ptr(), v.data_ptr(), v.data_ptr()
    last = sum((n - 1) * s for n, s in zip(v.shape, v.stride()) if n > 0)
    return v.untyped_storage().data_ptr(), v.data_ptr(), v.data_ptr() + (last + 1) * v.element_size()


def _groups(leaves):
    """union of operands whose byte ranges overlap: they are replayed inside one shared allocation"""
    spans = [_span(v) for _, v in leaves]
    parent = list(range(len(leaves)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in range(len(spans)):
        for j in range(i):
            si, sj = spans[i], spans[j]
            if si[0] == sj[0] and si[1] < sj[2] and sj[1] < si[2]:
                parent[find(i)] = find(j)
    return spans, [find(i) for i in range(len(leaves))]


def _enc(v, info):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, FMap):
        g, rel = info[id(v)]
        return ("F", _DTN[v.dtype], v.n, v.t, v.h, v.w, v.c, v.ld, v.c_off, g, rel)
    if torch.is_tensor(v):
        g, rel = info[id(v)]
        vals = tuple(int(x) for x in v.cpu().reshape(-1)) if v.dtype == torch.int32 and v.numel() <= 64 else None
        return ("T", _DTN[v.dtype], tuple(v.shape), tuple(v.stride()), g, rel, vals)
    if dataclasses.is_dataclass(v):
        return ("D", type(v).__name__, tuple((f.name, _enc(getattr(v, f.name), info)) for f in dataclasses.fields(v)))
    if isinstance(v, (list, tuple)):
        return ("S",) + tuple(_enc(x, info) for x in v)
    raise NotImplementedError(f"launch audit: cannot record an argument of type {type(v).__name__}")


def signature(be, method: str, bound: inspect.BoundArguments):
    """the geometry-only signature of one call: (method, ((arg, encoding), ...), groups, family)"""
    leaves = []
    for name, v in bound.arguments.items():
        _leaves(v, (name,), leaves)
    spans, root = _groups(leaves)
    gid, gbase = {}, {}
    for i, r in enumerate(root):
        gbase[r] = min(gbase.get(r, spans[i][1]), spans[i][1])
    groups = []
    info = {}
    for i, (_, v) in enumerate(leaves):
        r = root[i]
        if r not in gid:
            gid[r] = len(groups)
            members = [j for j in range(len(leaves)) if root[j] == r]
            groups.append((gbase[r] % 256, max(spans[j][2] for j in members) - gbase[r]))
        info[id(v)] = (gid[r], spans[i][1] - gbase[r])
    args = tuple((k, _enc(v, info)) for k, v in bound.arguments.items())
    fam = be.conv_family(bound.arguments["p"]) if method == "conv_igemm" and hasattr(be, "conv_family") else None
    return (method, args, tuple(groups), fam)


class Recorder:
    """Wraps a backend: forwards everything, stores the signature of every AUDITED call (tagged with `tag`)."""

    def __init__(self, backend, methods=AUDITED):
        self._be = backend
        self._methods = frozenset(methods)
        self.tag = None
        self.calls: Dict[tuple, set] = {}          # signature -> tags that bound it

    def __getattr__(self, name):
        attr = getattr(self._be, name)
        if name not in self._methods:
            return attr
        sig_of = inspect.signature(attr)

        def wrapped(*args, **kwargs):
            b = sig_of.bind(*args, **kwargs)
            b.apply_defaults()
            self.calls.setdefault(signature(self._be, name, b), set()).add(self.tag)
            return attr(*args, **kwargs)
        return wrapped


# ============================================================================= replay: buffers
class Buffers:
    """one raw allocation per recorded group, at the recorded 256-byte alignment, followed by GUARD bytes"""

    def __init__(self, groups, device):
        self.raw, self.views = [], []
        for align, nbytes in groups:
            raw = torch.empty(nbytes + GUARD + 512, dtype=torch.uint8, device=device)
            off = (align - raw.data_ptr()) % 256
            self.raw.append(raw)
            self.views.append(raw[off:off + nbytes + GUARD])

    def typed(self, g, rel, dtype, numel):
        es = torch.tensor([], dtype=dtype).element_size()
        return self.views[g][rel:rel + numel * es].view(dtype)


def _decode(e, bufs: Buffers):
    if not isinstance(e, tuple):
        return e
    if e[0] == "F":
        _, dt, n, t, h, w, c, ld, c_off, g, rel = e
        return FMap(bufs.typed(g, rel, _DT[dt], n * t * h * w * ld), n, t, h, w, c, ld, c_off)
    if e[0] == "T":
        _, dt, shape, stride, g, rel, _vals = e
        extent = 1 + sum((n - 1) * s for n, s in zip(shape, stride) if n > 0) if all(shape) else 0
        return torch.as_strided(bufs.typed(g, rel, _DT[dt], extent), shape, stride)
    if e[0] == "D":
        return _DC[e[1]](**{k: _decode(v, bufs) for k, v in e[2]})
    if e[0] == "S":
        return tuple(_decode(x, bufs) for x in e[1:])
    raise NotImplementedError(e[0])


def _fill(sig, bufs: Buffers, gen: torch.Generator):
    """seeded values: every group as N(0,1) of its first float operand's dtype (uint8 groups: random bytes), int32 index
    tensors as recorded"""
    first = {}

    def walk(e):
        if isinstance(e, tuple) and e and e[0] in ("F", "T"):
            g = e[9] if e[0] == "F" else e[4]
            first.setdefault(g, _DT[e[1]])
        elif isinstance(e, tuple):
            for x in e:
                walk(x)
    walk(sig[1])
    for g, v in enumerate(bufs.views):
        dt = first.get(g, torch.uint8)
        if dt == torch.uint8:
            v.copy_(torch.randint(0, 256, v.shape, generator=gen, device=gen.device, dtype=torch.int32).to(torch.uint8))
        elif dt in (torch.int32, torch.int64):
            v.zero_()
        else:
            es = torch.tensor([], dtype=dt).element_size()
            n = v.numel() // es
            v[: n * es].view(dt).copy_(torch.randn(n, generator=gen, device=gen.device).to(dt))


def _walk_ints(e, bufs):
    """write the recorded values of small int32 tensors (frame indices)"""
    if isinstance(e, tuple) and e and e[0] == "T":
        if e[6] is not None:
            _decode(e, bufs).copy_(torch.tensor(e[6], dtype=torch.int32).view(e[2]))
    elif isinstance(e, tuple):
        for x in e:
            _walk_ints(x, bufs)


# ============================================================================= replay: per-method restatements
class Out:
    """one written region: view(args) -> the region in a decoded argument set, checked against ref with bound (a, k)"""

    def __init__(self, name, view, ref, a, k, dtype, kind, alt=None, alt_mask=None, exact=False):
        self.name, self.view, self.ref, self.a, self.k, self.dtype, self.kind = name, view, ref, a, k, dtype, kind
        self.alt, self.alt_mask, self.exact = alt, alt_mask, exact


class _BitsOut(Out):
    """a ReLU bitmap: byte [pixel][c / vec] = the sign bits of the stored output"""

    def __init__(self, name, view, want, vec, stored):
        super().__init__(name, view, want, None, 0, torch.uint8, "bits", exact=True)
        self.vec, self.stored = vec, stored


def _kind(dtype):
    return "map_bf16" if dtype == torch.bfloat16 else "map_f32"


def _v5(f: FMap):
    return f.view5().to(F64)


def _ambiguous_mask(v, vb):
    """ReLU mask of a pre-activation v whose fp32 evaluation can be vb away: (mask, ambiguous)"""
    return v > 0, v.abs() <= vb


def _ref_conv_igemm(be, A):
    p: ConvPass = A["p"]
    X = _v5(p.x)
    W = p.w[: p.cout * p.wtaps * p.cin].view(p.cout, p.wtaps, p.cin)
    acc, a = ref64.conv(X, W, p.rows, p.gs, p.taps)
    K = p.cin * len(p.taps)
    ydt, outs = p.y.dtype, []
    sl = ref64.region(p.rows, p.os, p.oo)

    def ydest(q):
        return q["p"].y.view5()[:, sl[0], sl[1], sl[2]]
    old = ydest(A).to(F64)
    vec = 8 if ydt == torch.bfloat16 else 4
    if p.ep is not None:
        if p.stats is not None or p.bnb is not None or p.relu_out_bits is not None:
            raise NotImplementedError("epilogue combined with stats / bnb / out_relu_bits")
        e = p.ep
        v, av = acc, a
        if e.scale is not None:
            sc = e.scale[: p.cout].to(F64)
            v, av = v * sc, av * sc.abs()
        if e.shift is not None:
            v, av = v + e.shift[: p.cout].to(F64), av + e.shift[: p.cout].to(F64).abs()
        if p.accumulate:
            v, av = v + old, av + old.abs()
        if e.res is not None:
            r = _v5(e.res)
            ar = r.abs()
            if e.res_scale is not None:
                r, ar = r * e.res_scale[: p.cout].to(F64), ar * e.res_scale[: p.cout].to(F64).abs()
            if e.res_shift is not None:
                r, ar = r + e.res_shift[: p.cout].to(F64), ar + e.res_shift[: p.cout].to(F64).abs()
            v, av = v + r, av + ar
        if e.relu:
            bnd = ref64.elem_bound(v, av, K, torch.float32)
            m, amb = _ambiguous_mask(v, bnd)
            if e.relu_bits is not None:
                pix = p.y.pixels
                want = ref64.relu_bits_pack(m.reshape(pix, p.cout), vec)
                # the bitmap must be the sign of what the launch stored (the backward re-applies exactly that mask); the
                # stored y itself is held to float64 below.  Against the float64 sign, a pre-activation within a few fp32
                # roundings of zero can flip: seen once in ~2 M bytes on the pointwise family, with y inside its bound.
                outs.append(_BitsOut("relu_bits", lambda q: q["p"].ep.relu_bits[: pix * (p.cout // vec)], want, vec,
                                     lambda q: ydest(q)))
            v = v.clamp_min(0)
        outs.append(Out("y", ydest, v, av, K, ydt, _kind(ydt)))
        return outs
    res, ares = (old + acc, old.abs() + a) if p.accumulate else (acc, a)
    amb = alt = None
    if p.bnb is not None:
        b = p.bnb
        if p.stats is not None:
            raise NotImplementedError("bnb with stats")
        if b.y_bn is None:
            if p.relu_out_bits is None:
                raise NotImplementedError("bnb without y_bn needs out_relu_bits")
            mask = ref64.relu_bits_unpack(p.relu_out_bits, p.y.pixels, p.cout, vec).reshape(res.shape)
        elif b.mask_src is not None:
            mask = _v5(b.mask_src) > 0
        elif b.relu:
            v, vb = ref64.bn_pre(_v5(b.y_bn), b.scale[: p.cout], b.shift[: p.cout])
            mask, amb = _ambiguous_mask(v, vb)
        else:
            mask = torch.ones_like(res, dtype=torch.bool)
        if b.y_bn is not None and p.relu_out_bits is not None:
            raise NotImplementedError("bnb with y_bn and out_relu_bits")
        dz = res * mask
        if amb is not None:
            alt = res * (~mask)
        outs.append(Out("dz", ydest, dz, ares, K, ydt, _kind(ydt), alt=alt, alt_mask=amb))
        # the partial rows sum dz as stored (rounded to the map's dtype) or as the fp32 value before rounding: either passes
        dzs, dzu = ref64.rounded(dz, ydt).reshape(-1, p.cout), dz.reshape(-1, p.cout)
        adz = ares.reshape(-1, p.cout) * (mask.reshape(-1, p.cout) if amb is None else (mask | amb).reshape(-1, p.cout))
        mt = be.conv_igemm_mtiles(p)
        if b.y_bn is None:
            xh = torch.zeros(1, p.cout, dtype=F64, device=res.device)
            axh = xh
        else:
            yb = _v5(b.y_bn).reshape(-1, p.cout)
            mu, ist = b.mean[: p.cout].to(F64), b.invstd[: p.cout].to(F64)
            xh, axh = (yb - mu) * ist, (yb.abs() + mu.abs()) * ist.abs()
        st = torch.stack([dzs.sum(0), (dzs * xh).sum(0)], -1)
        su = torch.stack([dzu.sum(0), (dzu * xh).sum(0)], -1)
        sa = torch.stack([adz.sum(0), (adz * axh).sum(0)], -1)
        npx = res.numel() // p.cout
        outs.append(Out("bnb_partials", lambda q: _rows_sum(q["p"].bnb.partials, mt, p.cout), st, sa, _klen(npx, K),
                        torch.float32, "sum_f32_fused", alt=su, alt_mask=torch.ones_like(st, dtype=torch.bool)))
        outs.append(_untouched_rows("bnb_partials_tail", lambda q: q["p"].bnb.partials, mt, p.cout))
        return outs
    if p.relu_out_bits is not None:
        mask = ref64.relu_bits_unpack(p.relu_out_bits, p.y.pixels, p.cout, vec).reshape(res.shape)
        res, ares = res * mask, ares * mask
    outs.append(Out("y", ydest, res, ares, K, ydt, _kind(ydt)))
    if p.stats is not None:
        mt = be.conv_igemm_mtiles(p)
        flat, fa = acc.reshape(-1, p.cout), a.reshape(-1, p.cout)
        st = torch.stack([flat.sum(0), (flat * flat).sum(0)], -1)
        sa = torch.stack([fa.sum(0), (2 * flat.abs() * fa).sum(0)], -1)
        outs.append(Out("stats", lambda q: _rows_sum(q["p"].stats, mt, p.cout), st, sa, _klen(flat.shape[0], K),
                        torch.float32, "sum_f32"))
        outs.append(_untouched_rows("stats_tail", lambda q: q["p"].stats, mt, p.cout))
    return outs


def _klen(rows, k):
    """reduction length of a sum over `rows` values that are themselves k-term sums: (sqrt(rows) + sqrt(k))^2"""
    return (math.sqrt(rows) + math.sqrt(k)) ** 2


def _rows_sum(t, rows, c):
    return t[: rows * c * 2].view(rows, c, 2).to(F64).sum(0)


def _untouched_rows(name, view_full, rows, c):
    """rows >= `rows` of a partial-row buffer: checked by the untouched pass (marker Out with ref None)"""
    return Out(name, lambda q: view_full(q)[: rows * c * 2], None, None, 0, torch.float32, "written")


def _ref_conv_wgrad(be, A):
    p: WgradPass = A["p"]
    X, dY = _v5(p.x), _v5(p.dy)
    g, a = ref64.wgrad(X, dY, p.gs, p.taps, p.wtaps)
    n = p.cout * p.wtaps * p.cin
    base = p.dw[:n].to(F64).view(p.cout, p.wtaps, p.cin)
    rows = dY[..., 0].numel()
    outs = [Out("dw", lambda q: q["p"].dw[:n].view(p.cout, p.wtaps, p.cin), base + g, a + base.abs(), rows, torch.float32,
                "sum_f32")]
    if p.workspace is not None:
        outs.append(Out("workspace", lambda q: q["p"].workspace, None, None, 0, torch.float32, "scratch"))
    if p.dg_w is not None:
        Wd = p.dg_w[: p.cin * p.cout].view(p.cin, p.cout).to(F64)
        dg = dY @ Wd.t()
        adg = dY.abs() @ Wd.abs().t()
        outs.append(Out("dg_y", lambda q: q["p"].dg_y.view5(), dg, adg, p.cout, p.dg_y.dtype, _kind(p.dg_y.dtype)))
    return outs


def _ref_conv_pw_dual(be, A):
    x1, x2, y = A["x1"], A["x2"], A["y"]
    W1 = A["w1"][: y.c * x1.c].view(y.c, x1.c).to(F64)
    W2 = A["w2"][: y.c * x2.c].view(y.c, x2.c).to(F64)
    X1, X2 = _v5(x1), _v5(x2)
    v = X1 @ W1.t() + X2 @ W2.t()
    a = X1.abs() @ W1.abs().t() + X2.abs() @ W2.abs().t()
    if A["bias"] is not None:
        bb = A["bias"][: y.c].to(F64)
        v, a = v + bb, a + bb.abs()
    return [Out("y", lambda q: q["y"].view5(), v, a, x1.c + x2.c, y.dtype, _kind(y.dtype))]


def _stem_common(A, two_d):
    p: StemSrc = A["p"]
    y = A["y"] if "y" in A else A["dy"]
    if two_d:
        X = ref64.stem2d_x(p.src, y.dtype)
        cin, kt = p.src.shape[1], p.src.shape[2]
        taps = [(0, kh - 3, kw - 3, kh * 7 + kw) for kh in range(7) for kw in range(7)]
        rows, gs = (1, y.h, y.w), (1, 2, 2)
    else:
        X = ref64.stem_x(p.src, p.t_index, y.dtype)
        cin, kt = p.src.shape[1], p.kt
        taps = ref64.stem_taps(kt)
        rows, gs = (p.t_len, y.h, y.w), (1, 2, 2)
    return p, y, X, cin, kt, taps, rows, gs


def _ref_stem_fwd(be, A, two_d=False):
    p, y, X, cin, kt, taps, rows, gs = _stem_common(A, two_d)
    kp = stem_kp(cin, kt)
    W = ref64.stem_w(A["w"], y.c, cin, kt, kp)
    if two_d:                                     # (cout, 49, T*C): channel t*C + c = frame t, channel c
        W = W.view(y.c, kt, 49, cin).permute(0, 2, 1, 3).reshape(y.c, 49, kt * cin)
    acc, a = ref64.conv(X, W, rows, gs, taps)
    K = cin * kt * 49
    outs = [Out("y", lambda q: q["y"].view5(), acc, a, K, y.dtype, _kind(y.dtype))]
    if A["stats"] is not None:
        mt = (be.stem2d_tiles if two_d else be.stem_conv_tiles)(p, y)
        flat, fa = acc.reshape(-1, y.c), a.reshape(-1, y.c)
        st = torch.stack([flat.sum(0), (flat * flat).sum(0)], -1)
        sa = torch.stack([fa.sum(0), (flat.abs() * fa).sum(0) * 2], -1)
        outs.append(Out("stats", lambda q: _rows_sum(q["stats"], mt, y.c), st, sa, _klen(flat.shape[0], K), torch.float32,
                        "sum_f32"))
        outs.append(_untouched_rows("stats_tail", lambda q: q["stats"], mt, y.c))
    return outs


def _ref_stem_wgrad(be, A, two_d=False):
    p, dy, X, cin, kt, taps, rows, gs = _stem_common(A, two_d)
    nt = len(taps)
    g, a = ref64.wgrad(X, _v5(dy), gs, taps, nt)            # (cout, taps, cin or T*C)
    if two_d:
        g = g.view(dy.c, 49, kt, cin).permute(0, 2, 1, 3).reshape(dy.c, kt * 49, cin)
        a = a.view(dy.c, 49, kt, cin).permute(0, 2, 1, 3).reshape(dy.c, kt * 49, cin)
    kp = stem_kp(cin, kt)
    L = kt * cin * 56
    G, Ga = ref64.stem_w_layout(g, dy.c, cin, kt), ref64.stem_w_layout(a, dy.c, cin, kt)
    base = A["dw"][: dy.c * kp].view(dy.c, kp)[:, :L].to(F64)
    if not two_d:                                           # sfk_stem_conv_wgrad accumulates; the 2-D stem overwrites
        G, Ga = G + base, Ga + base.abs()
    def cols(t, lo, hi):                                    # [co][row of 8][kw]: kw < 7 taps, kw = 7 the padding column
        return t.view(t.shape[0], L // 8, 8)[:, :, lo:hi]

    def dwv(q):
        return q["dw"][: dy.c * kp].view(dy.c, kp)[:, :L]
    outs = [Out("dw", lambda q: cols(dwv(q), 0, 7), cols(G, 0, 7), cols(Ga, 0, 7), dy.pixels, torch.float32, "sum_f32")]
    if two_d:         # the 2-D stem overwrites dw: its padding is either left alone or written as zero
        z = torch.zeros_like(cols(G, 7, 8))
        outs.append(Out("dw_pad", lambda q: cols(dwv(q), 7, 8), z, z, 1, torch.float32, "pad", exact=True,
                        alt=cols(base, 7, 8), alt_mask=torch.ones_like(z, dtype=torch.bool)))
        if kp > L:
            tail = A["dw"][: dy.c * kp].view(dy.c, kp)[:, L:].to(F64)
            outs.append(Out("dw_rowpad", lambda q: q["dw"][: dy.c * kp].view(dy.c, kp)[:, L:], torch.zeros_like(tail),
                            torch.zeros_like(tail), 1, torch.float32, "pad", exact=True, alt=tail,
                            alt_mask=torch.ones_like(tail, dtype=torch.bool)))
    return outs


def _ref_bn_stats(be, A, nparts):
    y = A["y"]
    v = _v5(y).reshape(-1, y.c)
    st = torch.stack([v.sum(0), (v * v).sum(0)], -1)
    sa = torch.stack([v.abs().sum(0), (v * v).sum(0)], -1)
    return [Out("partials", lambda q: _rows_sum(q["partials"], nparts, y.c), st, sa, v.shape[0], torch.float32, "sum_f32"),
            _untouched_rows("partials_tail", lambda q: q["partials"], nparts, y.c)]


def _dz_reduce_outs(dz, amb_dz, y5, mean, invstd, c, nparts, name_view, dz_alt=None):
    """partial rows (sum dz, sum dz * xhat) of a BatchNorm backward reduce, as one Out (summed over rows)"""
    dzf = dz.reshape(-1, c)
    adz = dzf.abs() + (amb_dz.reshape(-1, c) if amb_dz is not None else 0)
    if y5 is None:
        s1 = torch.zeros(c, dtype=F64, device=dz.device)
        a1 = torch.zeros_like(s1)
    else:
        yf = y5.reshape(-1, c)
        mu, ist = mean[:c].to(F64), invstd[:c].to(F64)
        xh = (yf - mu) * ist
        s1 = (dzf * xh).sum(0)
        a1 = (adz * (yf.abs() + mu.abs()) * ist.abs()).sum(0)
    st = torch.stack([dzf.sum(0), s1], -1)
    sa = torch.stack([adz.sum(0), a1], -1)
    return [Out("partials", lambda q: _rows_sum(name_view(q), nparts, c), st, sa, dzf.shape[0], torch.float32, "sum_f32"),
            _untouched_rows("partials_tail", name_view, nparts, c)]


def _ref_bn_bwd_reduce(be, A, nparts):
    da, y, ms = A["da"], A["y"], A["mask_src"]
    c = da.c
    dav = _v5(da)
    amb = None
    if A["relu_bits"] is not None:
        if ms is not None:
            raise NotImplementedError("relu_bits with mask_src")
        vec = 8 if da.dtype == torch.bfloat16 else 4
        mask = ref64.relu_bits_unpack(A["relu_bits"], da.pixels, c, vec).reshape(dav.shape)
    elif ms is not None:
        mask = _v5(ms) > 0
    elif A["relu"]:
        v, vb = ref64.bn_pre(_v5(y), A["scale"][:c], A["shift"][:c])
        mask, amb = _ambiguous_mask(v, vb)
    else:
        mask = torch.ones_like(dav, dtype=torch.bool)
    dz = dav * mask
    outs = _dz_reduce_outs(dz, dav.abs() * amb if amb is not None else None, _v5(y) if y is not None else None,
                           A["mean"], A["invstd"], c, nparts, lambda q: q["partials"])
    if A["dz_out"] is not None:
        outs.append(Out("dz_out", lambda q: q["dz_out"].view5(), dz, torch.zeros_like(dz), 1, A["dz_out"].dtype,
                        _kind(A["dz_out"].dtype), alt=dav * (~mask) if amb is not None else None, alt_mask=amb))
    return outs


def _ref_bn_bwd_finalize(be, A):
    c, n, cnt = A["c"], A["nparts"], float(A["count"])
    pt = A["partials"][: n * c * 2].view(n, c, 2).to(F64)
    s, sa = pt.sum(0), pt.abs().sum(0)
    outs = []
    if A["dgamma"] is not None:
        b = A["dgamma"][:c].to(F64)
        outs.append(Out("dgamma", lambda q: q["dgamma"][:c], b + s[:, 1], b.abs() + sa[:, 1], n, torch.float32, "sum_f32"))
    if A["dbeta"] is not None:
        b = A["dbeta"][:c].to(F64)
        outs.append(Out("dbeta", lambda q: q["dbeta"][:c], b + s[:, 0], b.abs() + sa[:, 0], n, torch.float32, "sum_f32"))
    g, ist = A["gamma"][:c].to(F64), A["invstd"][:c].to(F64)
    cf = torch.stack([g * ist, s[:, 0] / cnt, s[:, 1] / cnt], -1)
    ca = torch.stack([(g * ist).abs(), sa[:, 0] / cnt, sa[:, 1] / cnt], -1)
    outs.append(Out("coef", lambda q: q["coef"][: c * 3].view(c, 3), cf, ca, n, torch.float32, "sum_f32"))
    if A["workspace"] is not None:
        outs.append(Out("workspace", lambda q: q["workspace"], None, None, 0, torch.float32, "scratch"))
    return outs


def _ref_bn_maxpool_fwd(be, A):
    y, out, k, s, p = A["y"], A["out"], A["k"], A["s"], A["p"]
    c = y.c
    v, vb = ref64.bn_pre(_v5(y), A["scale"][:c], A["shift"][:c])
    act = ref64.rounded(v.clamp_min(0), y.dtype)              # relu(y*scale + shift) rounded to the map's dtype
    best, arg = ref64.maxpool_fwd(act, k, s, p)
    aw, _ = ref64.maxpool_fwd(vb / ref64.EPS32, k, s, p)     # how far an fp32 evaluation of the window's values can be
    return [Out("out", lambda q: q["out"].view5(), best, aw, 1, out.dtype, _kind(out.dtype)),
            _ArgmaxOut("argmax", lambda q: q["argmax"][: best.numel()].view(best.shape), act, best, aw, k, s, p)]


class _ArgmaxOut(Out):
    """argmax is checked by what it points at: the activation at the chosen tap must equal the window maximum"""

    def __init__(self, name, view, act, best, vb, k, s, p):
        super().__init__(name, view, None, None, 0, torch.uint8, "argmax")
        self.act, self.best, self.vb, self.k, self.s, self.p = act, best, vb, k, s, p


def _stem_tail_da(A):
    d_out, y = A["d_out"], A["y"]
    arg = A["argmax"][: d_out.pixels * d_out.c].view(d_out.n, d_out.t, d_out.h, d_out.w, d_out.c)
    da = ref64.maxpool_bwd(_v5(d_out), arg, y.h, y.w, 3, 2, 1)
    return ref64.rounded(da, y.dtype)                         # rounded to the map's dtype, as sfk_maxpool_bwd stores it


def _ref_bn_maxpool_bwd(be, A, nparts=None, apply=False):
    y = A["y"]
    c = y.c
    da = _stem_tail_da(A)
    v, vb = ref64.bn_pre(_v5(y), A["scale"][:c], A["shift"][:c])
    mask, amb = _ambiguous_mask(v, vb)
    dz = da * mask
    if not apply:
        return _dz_reduce_outs(dz, da.abs() * amb, _v5(y), A["mean"], A["invstd"], c, nparts, lambda q: q["partials"])
    cf = A["coef"][: c * 3].view(c, 3).to(F64)
    xh = (_v5(y) - A["mean"][:c].to(F64)) * A["invstd"][:c].to(F64)
    r = cf[:, 0] * (dz - cf[:, 1] - xh * cf[:, 2])
    alt = cf[:, 0] * (da * (~mask) - cf[:, 1] - xh * cf[:, 2])
    a = cf[:, 0].abs() * (dz.abs() + cf[:, 1].abs() + (_v5(y).abs() + A["mean"][:c].to(F64).abs())
                          * A["invstd"][:c].to(F64).abs() * cf[:, 2].abs())
    return [Out("dy", lambda q: q["dy"].view5(), r, a, 4, A["dy"].dtype, _kind(A["dy"].dtype), alt=alt, alt_mask=amb)]


_REFS = {
    "conv_igemm": lambda be, A, np_: _ref_conv_igemm(be, A),
    "conv_wgrad": lambda be, A, np_: _ref_conv_wgrad(be, A),
    "conv_pw_dual": lambda be, A, np_: _ref_conv_pw_dual(be, A),
    "stem_conv_fwd": lambda be, A, np_: _ref_stem_fwd(be, A),
    "stem_conv_wgrad": lambda be, A, np_: _ref_stem_wgrad(be, A),
    "stem2d_fwd": lambda be, A, np_: _ref_stem_fwd(be, A, two_d=True),
    "stem2d_wgrad": lambda be, A, np_: _ref_stem_wgrad(be, A, two_d=True),
    "bn_stats": lambda be, A, np_: _ref_bn_stats(be, A, np_),
    "bn_bwd_reduce": lambda be, A, np_: _ref_bn_bwd_reduce(be, A, np_),
    "bn_bwd_finalize": lambda be, A, np_: _ref_bn_bwd_finalize(be, A),
    "bn_maxpool_fwd": lambda be, A, np_: _ref_bn_maxpool_fwd(be, A),
    "bn_maxpool_bwd_reduce": lambda be, A, np_: _ref_bn_maxpool_bwd(be, A, np_),
    "bn_maxpool_bwd_apply": lambda be, A, np_: _ref_bn_maxpool_bwd(be, A, apply=True),
}


# ============================================================================= replay: inputs with meaning
def _prepare_inputs(method, A, gen, be):
    """values a random fill cannot stand for: filters N(0, 1/K), stem-layout padding zero, positive invstd, and a valid
    argmax (the maxpool argmax of the stem tail, from the restated forward)"""

    def rnd(t, std):
        t.copy_((torch.randn(t.shape, generator=gen, device=gen.device) * std).to(t.dtype).to(t.device))

    if method == "conv_igemm":
        p = A["p"]
        rnd(p.w[: p.cout * p.wtaps * p.cin], 1.0 / math.sqrt(p.cin * len(p.taps)))
        if p.bnb is not None and p.bnb.invstd is not None:
            p.bnb.invstd.abs_().add_(0.25)
    elif method == "conv_wgrad":
        p = A["p"]
        if p.dg_w is not None:
            rnd(p.dg_w[: p.cin * p.cout], 1.0 / math.sqrt(p.cout))
    elif method == "conv_pw_dual":
        y = A["y"]
        rnd(A["w1"][: y.c * A["x1"].c], 1.0 / math.sqrt(A["x1"].c + A["x2"].c))
        rnd(A["w2"][: y.c * A["x2"].c], 1.0 / math.sqrt(A["x1"].c + A["x2"].c))
    elif method in ("stem_conv_fwd", "stem2d_fwd"):
        p, y = A["p"], A["y"]
        cin = p.src.shape[1]
        kt = p.src.shape[2] if method == "stem2d_fwd" else p.kt
        kp = stem_kp(cin, kt)
        w = A["w"][: y.c * kp].view(y.c, kp)
        rnd(w, 1.0 / math.sqrt(cin * kt * 49))
        w[:, kt * cin * 56:] = 0
        w[:, : kt * cin * 56].view(y.c, -1, 8)[:, :, 7] = 0
    if method in ("bn_bwd_reduce", "bn_bwd_finalize", "bn_maxpool_bwd_reduce", "bn_maxpool_bwd_apply"):
        if A.get("invstd") is not None:
            A["invstd"].abs_().add_(0.25)
    if method in ("bn_maxpool_bwd_reduce", "bn_maxpool_bwd_apply"):
        y, d_out = A["y"], A["d_out"]
        c = y.c
        v, _ = ref64.bn_pre(_v5(y), A["scale"][:c], A["shift"][:c])
        _, arg = ref64.maxpool_fwd(ref64.rounded(v.clamp_min(0), y.dtype), 3, 2, 1)
        A["argmax"][: arg.numel()].copy_(arg.reshape(-1))


# ============================================================================= replay
class Replay:
    """the outcome of one replayed signature"""

    def __init__(self, sig, family, verdicts, untouched_ok, untouched_bad, route=None, ambiguous=0.0, args=None):
        self.sig, self.family, self.verdicts = sig, family, verdicts
        self.untouched_ok, self.untouched_bad = untouched_ok, untouched_bad
        self.route = route                # what the backend's route query says of the REPLAYED descriptor (None: no query)
        self.ambiguous = ambiguous        # largest share of a map's elements whose ReLU sign the reference cannot decide
        self.args = args                  # the decoded arguments after the launch (for a second, bit-compared run)

    @property
    def ok(self):
        return self.untouched_ok and all(v.ok for v in self.verdicts)

    @property
    def worst(self):
        return max([v.worst for v in self.verdicts] + [0.0])

    @property
    def agg(self):
        return max([v.agg / v.agg_bound for v in self.verdicts] + [0.0])     # (0 for a map judged by its elements alone)


def describe(sig) -> str:
    """one short line: the method and its main maps"""
    method, args = sig[0], dict(sig[1])
    parts = []

    def fm(e):
        return f"{e[1]}[{e[2]}x{e[3]}x{e[4]}x{e[5]}x{e[6]}{'/ld' + str(e[7]) if e[7] != e[6] else ''}" \
               f"{'+' + str(e[8]) if e[8] else ''}]"
    for k, e in args.items():
        if isinstance(e, tuple) and e and e[0] == "F":
            parts.append(f"{k}={fm(e)}")
        elif isinstance(e, tuple) and e and e[0] == "D":
            d = dict(e[2])
            for f in ("x", "y", "dy", "dg_y"):
                if isinstance(d.get(f), tuple) and d[f] and d[f][0] == "F":
                    parts.append(f"{f}={fm(d[f])}")
            for f in ("rows", "gs", "os", "oo"):
                if f in d:
                    parts.append(f"{f}={tuple(d[f][1:]) if isinstance(d[f], tuple) else d[f]}")
            if "taps" in d:
                parts.append(f"taps={len(d['taps']) - 1}")
            opt = [f for f in ("stats", "bnb", "relu_out_bits", "ep", "workspace", "dg_w", "t_index")
                   if d.get(f) is not None]
            if d.get("accumulate"):
                opt.append("acc")
            if opt:
                parts.append("+" + ",".join(opt))
            if "src" in d:
                parts.append(f"src={d['src'][2]}")
    return f"{method} " + " ".join(parts)


def replay(sig, be, device, seed: int = 0) -> Replay:
    method, args, groups, family = sig
    if method not in _REFS:
        raise NotImplementedError(f"launch audit: no float64 restatement of {method}")
    gen = torch.Generator(device=device).manual_seed(seed)
    bufs = Buffers(groups, device)
    _fill(sig, bufs, gen)
    _walk_ints(args, bufs)
    A = {k: _decode(e, bufs) for k, e in args}
    _prepare_inputs(method, A, gen, be)
    fam = be.conv_family(A["p"]) if method == "conv_igemm" and hasattr(be, "conv_family") else None
    route = None
    if method == "conv_igemm" and hasattr(be, "conv_route"):
        route = be.conv_route(A["p"])
    elif method == "conv_wgrad" and hasattr(be, "conv_wgrad_route"):
        route = be.conv_wgrad_route(A["p"])
    before = Buffers(groups, device)
    for b, a in zip(before.views, bufs.views):
        b.copy_(a)
    B = {k: _decode(e, before) for k, e in args}         # the inputs as they were, in their own copy
    res = getattr(be, method)(**A)
    run, nparts = (res if isinstance(res, tuple) else (res, None))
    run(torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    outs = _REFS[method](be, B, nparts)
    verdicts = []
    for o in outs:
        if o.ref is None:
            continue
        if isinstance(o, _ArgmaxOut):
            verdicts.append(_check_argmax(o, o.view(A)))
            continue
        if isinstance(o, _BitsOut):
            st = o.stored(A)
            sign = ref64.relu_bits_pack((st.reshape(-1, st.shape[-1]) > 0), o.vec)
            got = o.view(A)
            bad = int((got != sign).sum())
            flips = int((got != o.ref).sum())
            verdicts.append(ref64.Verdict(o.name, o.kind, 0.0 if bad == 0 else float("inf"), 0.0, 1.0, got.numel(),
                                          f"{bad} bytes disagree with the stored sign, {flips} with the float64 sign"))
            continue
        got = o.view(A)
        if o.exact:
            g = got.to(F64)
            ok = (g == o.ref.to(F64))
            if o.alt is not None:
                ok |= o.alt_mask & (g == o.alt.to(F64))
            bad = int((~ok).sum())
            where = None
            if bad:
                i = int(torch.nonzero(~ok.reshape(-1))[0])
                where = f"{bad} bad, first {i}: got {int(g.reshape(-1)[i])} want {int(o.ref.reshape(-1)[i])}"
            verdicts.append(ref64.Verdict(o.name, o.kind, 0.0 if bad == 0 else float("inf"), 0.0, 1.0, g.numel(), where))
            continue
        verdicts.append(ref64.judge(o.name, got, o.ref, o.a, o.k, o.dtype, o.kind, alt=o.alt, alt_mask=o.alt_mask))
    # untouched: restore every written region from the snapshot; then the whole allocation must equal the snapshot
    after = Buffers(groups, device)
    for b, a in zip(after.views, bufs.views):
        b.copy_(a)
    Aft = {k: _decode(e, after) for k, e in args}
    for o in outs:
        o.view(Aft).copy_(o.view(B))
    bad = [i for i, (x, y) in enumerate(zip(after.views, before.views)) if not torch.equal(x, y)]
    amb = max([float(o.alt_mask.double().mean()) for o in outs
               if o.alt_mask is not None and o.kind.startswith("map_") and o.alt_mask.numel()] + [0.0])
    return Replay(sig, fam, verdicts, not bad, bad, route, amb, A)


def _check_argmax(o: _ArgmaxOut, arg: torch.Tensor) -> ref64.Verdict:
    """the activation at the kernel's chosen tap equals the window maximum (ties: any maximal tap passes)"""
    n, t, ho, wo, c = o.best.shape
    kh, kw = arg.long() // o.k, arg.long() % o.k
    hi = torch.arange(ho, device=arg.device).view(1, 1, -1, 1, 1) * o.s - o.p + kh
    wi = torch.arange(wo, device=arg.device).view(1, 1, 1, -1, 1) * o.s - o.p + kw
    h, w = o.act.shape[2], o.act.shape[3]
    inside = (hi >= 0) & (hi < h) & (wi >= 0) & (wi < w) & (arg.long() < o.k * o.k)
    hi, wi = hi.clamp(0, h - 1), wi.clamp(0, w - 1)
    ni = torch.arange(n, device=arg.device).view(-1, 1, 1, 1, 1)
    ti = torch.arange(t, device=arg.device).view(1, -1, 1, 1, 1)
    ci = torch.arange(c, device=arg.device).view(1, 1, 1, 1, -1)
    picked = o.act[ni, ti, hi, wi, ci]
    tol = ref64.elem_bound(o.best, o.vb, 1, torch.bfloat16)
    ok = inside & ((picked - o.best).abs() <= tol)
    bad = int((~ok).sum())
    return ref64.Verdict("argmax", "argmax", 0.0 if bad == 0 else float("inf"), 0.0, 1.0, arg.numel())


# ============================================================================= plans of the production geometries
def record_plans(backend, device, geometries) -> Recorder:
    """Build (never run) the default bf16 train plan of each geometry with a Recorder around `backend`; the models and
    their plans are dropped before this returns.  geometries: name -> callable(backend, device) -> (model, x_slow, x_fast,
    slow_t_index)."""
    import gc
    rec = Recorder(backend)
    for name, make in geometries.items():
        rec.tag = name
        model, xs, xf, idx = make(rec, device)
        model.engine._plan_for(xs, xf, idx, True)
        del model, xs, xf, idx
        gc.collect()
        if torch.device(device).type == "cuda":
            torch.cuda.empty_cache()
    return rec


def geometry_bench(be, device):
    from video_classification_amd.slowfast import pack_pathway_index, slowfast_r50_8x8
    m = slowfast_r50_8x8(400, dtype=torch.bfloat16, device=device, backend=be, seed=0)
    frames = torch.empty(32, 3, 32, 224, 224, dtype=torch.bfloat16, device=device)
    return m, frames, frames, pack_pathway_index(32, 4, device)


def geometry_res2d(be, device):
    from video_classification_amd.slowfast import resnet50_2d_engine
    m = resnet50_2d_engine(249, clip_len=10, crop=128, dtype=torch.bfloat16, device=device, backend=be, seed=0)
    x = torch.empty(60, 10 * 5, 128, 128, dtype=torch.bfloat16, device=device)
    return m, m.engine.input_view(x), None, None


def geometry_v2(be, device):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=249, input_channels=(5, 2), stem_dim_outs=(64, 8), depth=50,
                         head_pool_kernels=((4, 2, 2), (4, 2, 2)))
    m = SlowFast(spec, dtype=torch.bfloat16, device=device, backend=be, seed=0)
    xs = torch.empty(10, 5, 20, 192, 192, dtype=torch.bfloat16, device=device)
    xf = torch.empty(10, 2, 20, 192, 192, dtype=torch.bfloat16, device=device)
    return m, xs, xf, None


PRODUCTION = {"bench": geometry_bench, "res2d": geometry_res2d, "v2": geometry_v2}
