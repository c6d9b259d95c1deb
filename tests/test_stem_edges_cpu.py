"""The stem edge table (tests/stem_edges.py) without a GPU:
  * closure -- the host-only route queries (sfk_stem_conv_fwd_route / sfk_stem_conv_wgrad_route: the launch code run dry) work
    on CPU tensors and need no filter; the routes the table reaches are exactly include/sfk.h's SFK_STEM_ROUTES, every case
    reaches the route (and the work items / workgroups) it declares, every refused case returns the status it declares;
  * the restatements -- launch_audit's float64 stem forward and filter gradient agree with torch.nn.functional.conv3d and its
    autograd in float64 to 1e-12 on every case, so the reference of the GPU test is the operation the header names;
  * the reference alone -- every case replayed on the torch emulation is inside every bound, so a GPU failure is the kernel's;
  * mutations -- the ways a stem kernel goes wrong at an edge, each played on the emulated result, each refused."""
import dataclasses

import pytest
import torch

import launch_audit as la
import ref64
import stem_edges as E
from emu_backend import EmuBackend
from emu_stem2d import EmuStem2dBackend
from emu_u8stem import EmuU8StemBackend
from emu_u8stem_pool import EmuU8StemPoolBackend
from video_classification_amd._lib import FMap, HipBackend, SfkError, StemSrc, stem_kp

F64 = torch.float64
LIVE = [c for c in E.CASES if c.status == 0]
REFUSED = [c for c in E.CASES if c.status < 0]


def _emu_u8(case):
    return EmuU8StemPoolBackend() if case.pool else EmuU8StemBackend()


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def _query(hip, case):
    p, m, _ = E.bound(case, hip)
    try:
        return hip.stem_route(p, m, E.is_wgrad(case.method))
    except SfkError as e:
        return int(str(e).rstrip(")").rsplit("(", 1)[1])


def test_every_declared_route_is_reported_and_the_table_covers_the_header(hip):
    routes = E.header_routes()
    assert len(routes) == 30
    seen, bad = set(), []
    for c in E.CASES:
        if c.method.startswith("stem2d"):
            assert c.route is None                             # (one instantiation per dtype pair: no query)
            continue
        r = _query(hip, c)
        if c.status < 0:
            if r != c.status:
                bad.append((c.name, "status", c.status, r))
            continue
        if isinstance(r, int):
            bad.append((c.name, "refused", r))
            continue
        route, units, grid = r
        seen.add(route)
        if route != c.route:
            bad.append((c.name, E.route_name(c.route), E.route_name(route)))
        if (c.units is not None and units != c.units) or (c.grid is not None and grid != c.grid) or \
                (c.wrap is not None and (units > grid) != c.wrap):
            bad.append((c.name, "units / grid", c.units, c.grid, c.wrap, units, grid))
    assert not bad, bad
    assert seen == set(routes), ([routes[r] for r in set(routes) - seen], [hex(r) for r in seen - set(routes)])


def test_the_table_has_the_edges_it_claims(hip):
    """layout rules of the table: sliced maps, misaligned bases, poisoned statistics rows, wrapped unit loops per kernel"""
    wraps = set()
    for c in E.CASES:
        p, m, sig = E.bound(c, hip)
        assert m.ld > m.c and m.c_off > 0, c.name
        assert m.buf.data_ptr() % 256 == 16, c.name
        if c.route is not None and c.route >> 8 in (E.SK["V4"], E.SK["V2"], E.SK["S4"], E.SK["WGV2"]):
            assert p.src.data_ptr() % 16 == 0 and (p.src.data_ptr() % 256 == 16 or p.src.storage_offset()), c.name
        args = dict(sig[1])
        for k in ("w", "dw", "stats"):
            if args.get(k) is not None:
                assert sig[2][args[k][4]][0] == (0 if k == "stats" else 16), (c.name, k)
        if c.route == E.S4:
            assert m.ld % 8 == 0 and m.c_off % 8 == 0
        if c.wrap:
            wraps.add(c.route >> 8)
        assert m.pixels <= 129 * 2 * 16 * 20, c.name
    assert wraps == set(E.SK.values())                         # every kernel has a case with more work items than workgroups
    for kern in ("V4", "V2"):
        assert any(c.route is not None and c.route >> 8 == E.SK[kern] and "coff4" in c.name for c in E.CASES)


def test_route_query_needs_no_filter_and_returns_the_status_of_a_bad_descriptor(hip):
    p, m, _ = E.bound(E.BY_NAME["v4_k5_c8_t2_7x4"], hip)
    assert hip.stem_route(p, m)[0] == E.V5
    bad = FMap(m.buf, m.n, m.t - 1, m.h, m.w, m.c, m.ld, m.c_off)             # t_out != the frames the source selects
    with pytest.raises(SfkError, match=r"sfk_stem_conv_fwd_route: .*\(-1\)"):
        hip.stem_route(p, bad)
    with pytest.raises(SfkError, match=r"sfk_stem_conv_wgrad_route: .*\(-1\)"):
        hip.stem_route(p, bad, True)
    odd = FMap(torch.zeros(m.buf.numel() + 2, dtype=m.dtype)[2:], m.n, m.t, m.h, m.w, m.c, m.ld, m.c_off)             # the map 4 bytes off
    with pytest.raises(SfkError, match=r"\(-2\)"):
        hip.stem_route(p, odd)
    # the fast routes hand over when the source loses its 16-byte rows: one element off is the generic kernel
    q = StemSrc(torch.zeros(p.src.numel() + 8, dtype=p.src.dtype)[1:1 + p.src.numel()].view(p.src.shape), None, p.kt)
    assert hip.stem_route(q, m)[0] == E.SR("GENERIC", 1, 1, 1)


# ----------------------------------------------------------------------------- the restatements against torch's conv3d
def _conv3d_f64(A, method):
    """conv3d / its autograd in float64 on the filled arguments: what launch_audit's first Out must equal"""
    two_d = method.startswith("stem2d")
    p, m = A["p"], A["y"] if "y" in A else A["dy"]
    x = p.src.to(m.dtype).to(F64)
    if p.t_index is not None:
        x = x.index_select(2, p.t_index.long())
    cin, kt = x.shape[1], (x.shape[2] if two_d else p.kt)
    pad = (0 if two_d else kt // 2, 3, 3)
    if not E.is_wgrad(method):
        wt = EmuBackend.stem_weight_from_layout(A["w"].to(F64), m.c, cin, kt).to(F64)
        return torch.nn.functional.conv3d(x, wt, None, (1, 2, 2), pad).permute(0, 2, 3, 4, 1)
    with torch.enable_grad():
        wt = torch.zeros(m.c, cin, kt, 7, 7, dtype=F64, requires_grad=True)
        torch.nn.functional.conv3d(x, wt, None, (1, 2, 2), pad).backward(m.view5().to(F64).permute(0, 4, 1, 2, 3))
    g = wt.grad.permute(0, 2, 1, 3, 4).reshape(m.c, kt * cin * 7, 7)                        # [co][(f, ci, kh)][kw]
    if not two_d:
        kp = stem_kp(cin, kt)
        g = g + A["dw"][: m.c * kp].view(m.c, kp)[:, : kt * cin * 56].to(F64).view(m.c, -1, 8)[:, :, :7]
    return g


@pytest.mark.parametrize("case", LIVE, ids=lambda c: c.name)
def test_the_restatement_is_conv3d_in_float64(case):
    be = EmuStem2dBackend()
    _, _, sig = E.bound(case, be)
    A, _ = E.filled(sig, be, "cpu", case.seed)
    out = la._REFS[case.method](be, A, None)[0]
    want = _conv3d_f64(A, case.method)
    assert out.ref.shape == want.shape
    assert float((out.ref - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize("case", LIVE, ids=lambda c: c.name)
def test_the_reference_alone_is_inside_every_bound(case):
    be = EmuStem2dBackend()
    _, _, sig = E.bound(case, be)
    r = la.replay(sig, be, "cpu", seed=case.seed)
    assert r.ok, (r.verdicts, r.untouched_bad)


@pytest.mark.parametrize("case", E.U8, ids=lambda c: c.name)
def test_the_u8_reference_alone_is_inside_every_bound(case):
    r, _ = E.u8_run(case, _emu_u8(case), "cpu")
    assert r.ok, (r.verdicts, r.untouched_bad)


def test_the_u8_table_covers_every_source_tag_and_fragment_count():
    fwd = [c for c in E.U8 if c.kind == "3d" and not c.wg]
    tags = ("Lut", "Pix5", "Pix15", "PoolLut", "PoolPix5", "PoolPix15")
    assert {(c.tag, c.mdt) for c in fwd} == {(t, d) for t in tags for d in (E.BF16, E.F32)}
    assert {(c.tag, {1: 1, 2: 2, 3: 4, 4: 4}[(c.cout + 15) // 16]) for c in fwd} == {(t, f) for t in tags for f in (1, 2, 4)}
    for pool in (False, True):
        some = [c for c in E.U8 if c.pool == pool]
        assert {c.crop for c in some} == {None, "zero", "max", "random"} and {c.s for c in some} == {18, 34, 70}
        assert any(c.pitch == c.c for c in some) and any(c.pitch == 21 and c.c0 > 0 for c in some) and any(c.ti for c in some)
        assert {c.method for c in some} == {("u8p" if pool else "u8") + m for m in
                                            ("stem_conv_fwd", "stem_conv_wgrad", "stem2d_fwd", "stem2d_wgrad")}
    assert all(c.missing for c in E.U8 if c.pool) and any(c.kt == 3 and c.missing for c in E.U8 if c.pool)


# ----------------------------------------------------------------------------- mutations
def _mutant(method, pre=None, snap=None, post=None):
    """an EmuStem2dBackend whose `method` runs on pre(args) and / or has its outputs tampered with by post(args, snap(args));
    args: the call's arguments by name"""
    names = ("p", "dy", "dw") if E.is_wgrad(method) else ("p", "w", "y", "stats")

    class M(EmuStem2dBackend):
        pass

    def call(self, *args, **kw):
        a = {**dict(zip(names, args)), **kw}
        run = getattr(EmuStem2dBackend, method)(self, **(pre(a) if pre else a))

        def r(stream):
            s = snap(a) if snap else None
            run(stream)
            if post:
                post(a, s)
        return r
    setattr(M, method, call)
    return M()


def _reslice(f: FMap, c_off: int) -> FMap:
    return FMap(f.buf, f.n, f.t, f.h, f.w, f.c, f.ld, c_off)


def _pad_frame_is_frame_0(a, _):
    """leading temporal padding reads frame 0 instead of zeros (a clamped frame index)"""
    p, y = a["p"], a["y"]
    pt = p.kt // 2
    x = p.src if p.t_index is None else p.src.index_select(2, p.t_index.long())
    ext = torch.cat([x[:, :, :1]] * pt + [x, torch.zeros_like(x[:, :, :pt])], 2)
    ye = FMap(torch.zeros(y.n * (y.t + 2 * pt) * y.h * y.w * y.c, dtype=y.dtype), y.n, y.t + 2 * pt, y.h, y.w, y.c)
    EmuBackend().stem_conv_fwd(StemSrc(ext, None, p.kt), a["w"], ye, None)(0)
    y.view5().copy_(ye.view5()[:, pt:pt + y.t])


def _past_the_map(a, _):
    """a half tile of 8 rows stores its row 7 although ho is 7: in the last frame that is the pixel record behind the map"""
    y = a["y"]
    behind = torch.as_strided(y.buf, (y.c,), (1,), y.buf.storage_offset() + y.buf.numel() + y.c_off)
    behind.fill_(1.0)


def _unit_stats_twice(a, _):
    y, st = a["y"], a["stats"]
    v = y.view5()[0, 0, :8, :16].float().reshape(-1, y.c)                      # the first unit's half tile of frame 0
    row = st[y.c * 2: y.c * 4].view(y.c, 2)
    row[:, 0] += v.sum(0)
    row[:, 1] += (v * v).sum(0)


def _stats_row_past_mt(a, _):
    mt = EmuBackend().stem_conv_tiles(a["p"], a["y"])
    a["stats"][mt * a["y"].c * 2] = 3.0


def _channels_4_to_7(a, _):
    y = a["y"]
    y.buf.view(-1, y.ld)[:, y.c_off + 4: y.c_off + 8] = 1.0


MUTATIONS = {
    "trailing half-pair frame dropped": ("v4_k5_c4_t3_1x12_coff4", dict(
        snap=lambda a: a["y"].view5()[:, -1].clone(), post=lambda a, s: a["y"].view5()[:, -1].copy_(s))),
    "temporal-padding frame read as frame 0": ("v4_k5_c8_t2_7x4", dict(post=_pad_frame_is_frame_0)),
    "t_index ignored": ("v4_k5_c8_tindex_repeats", dict(
        pre=lambda a: {**a, "p": StemSrc(a["p"].src[:, :, : a["p"].t_len], None, a["p"].kt)})),
    "last tile column dropped": ("v4_k3_c8_t17_9x20", dict(
        snap=lambda a: a["y"].view5()[:, :, :, -1].clone(), post=lambda a, s: a["y"].view5()[:, :, :, -1].copy_(s))),
    "last tile column duplicated": ("s4_t5_9x20", dict(
        post=lambda a, s: a["y"].view5()[:, :, :, -1].copy_(a["y"].view5()[:, :, :, -2]))),
    "row past ho written in a half tile": ("s4_t2_7x4", dict(post=_past_the_map)),
    "c_off + 4": ("v4_k5_c4_t3_1x12_coff4", dict(pre=lambda a: {**a, "y": _reslice(a["y"], a["y"].c_off + 4)})),
    "write into kw == 7": ("wgv2_k1_t1_7x4", dict(
        post=lambda a, s: a["dw"][: 8 * stem_kp(3, 1)].view(8, -1)[:, 7].fill_(0.0))),
    "dw overwritten instead of accumulated": ("wgv2_k5_t2_18x20", dict(
        snap=lambda a: a["dw"].clone(), post=lambda a, s: a["dw"].sub_(s))),
    "one unit's statistics added twice": ("v4_k3_c8_t17_9x20", dict(post=_unit_stats_twice)),
    "statistics row past mt written": ("v2_k5_c8_18x20", dict(post=_stats_row_past_mt)),
    "cout 4 writing channels 4..7": ("v4_k5_c4_t3_1x12_coff4", dict(post=_channels_4_to_7)),
    "generic: last output row dropped": ("gen_c5k1_f32_from_f32_co20", dict(
        snap=lambda a: a["y"].view5()[:, :, -1].clone(), post=lambda a, s: a["y"].view5()[:, :, -1].copy_(s))),
}


@pytest.mark.parametrize("what", list(MUTATIONS), ids=lambda s: s.replace(" ", "_"))
def test_replay_refuses_the_mutation(what):
    name, how = MUTATIONS[what]
    case = E.BY_NAME[name]
    _, _, sig = E.bound(case, EmuStem2dBackend())
    assert la.replay(sig, EmuStem2dBackend(), "cpu", seed=case.seed).ok
    r = la.replay(sig, _mutant(case.method, **how), "cpu", seed=case.seed)
    assert not r.ok, (what, r.verdicts)


@pytest.mark.parametrize("pool", [False, True], ids=["stacked", "pooled"])
def test_the_u8_check_refuses_a_crop_shift_off_by_one(pool):
    case = next(c for c in E.U8 if c.pool == pool and c.crop == "random" and not c.wg and c.kind == "3d")
    be = _emu_u8(case)
    assert E.u8_run(case, be, "cpu")[0].ok
    r, _ = E.u8_run(case, be, "cpu", crop_delta=1)
    assert not r.ok, r.verdicts
    zero = next(c for c in E.U8 if c.pool == pool and c.crop == "zero" and not c.wg)
    assert not E.u8_run(zero, be, "cpu", crop_delta=1)[0].ok


def test_refused_cases_are_declared_for_both_entry_points():
    assert len(REFUSED) >= 10 and {c.status for c in REFUSED} == {E.UNSUPPORTED}
    assert {c.method for c in REFUSED} == {"stem_conv_fwd", "stem_conv_wgrad", "stem2d_fwd", "stem2d_wgrad"}
    assert len(LIVE) >= 90 and len(dataclasses.fields(E.Case)) == 10
