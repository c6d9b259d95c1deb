"""The conv / filter-gradient edge table (tests/conv_edges.py) without a GPU:
  * closure -- the host-only route queries (sfk_conv_igemm_route / sfk_conv_wgrad_route: the launch code run dry) work on CPU
    tensors; the routes the table reaches are exactly the lists include/sfk.h declares, every case reaches the route it
    declares, and sfk_conv_igemm_family / _mtiles agree with the route;
  * the reference alone -- every case replayed on the torch restatement of the contract (EmuBackend) is inside every bound of
    launch_audit.replay, so a GPU failure of a case is the kernel's;
  * mutations -- the ways a kernel goes wrong at an edge, each played by an EmuBackend subclass, each refused by replay."""
import ctypes as C
import dataclasses

import pytest
import torch

import conv_edges as E
import launch_audit as la
import ref64
from video_classification_amd import _lib
from video_classification_amd._lib import FMap, HipBackend

AMB_CAP = 1e-3            # share of ambiguous ReLU signs a case may excuse (bn_ref64.AMB_CAP)


@pytest.fixture(scope="module")
def hip():
    return HipBackend()


def _bound(case, be):
    rec = la.Recorder(be)
    q = case.bind(rec, "cpu")
    (sig,) = rec.calls
    return q, sig


def test_every_declared_route_is_reported_and_the_table_covers_the_header(hip):
    ig, wg = E.header_routes()
    assert len(ig) >= 60 and len(wg) >= 25 and not set(ig) & set(wg)
    seen_i, seen_w, bad = set(), set(), []
    for c in E.CASES:
        q, _ = _bound(c, hip)
        if c.method == "conv_igemm":
            r = hip.conv_route(q)
            seen_i.add(r)
            if r != c.route:
                bad.append((c.name, E.route_name(c.route), E.route_name(r)))
            kern, bm = (r >> 24) & 15, (r >> 15) & 511
            if hip.conv_family(q) != E.FAMILY_OF_KERNEL[kern]:
                bad.append((c.name, "family", hip.conv_family(q)))
            m = q.x.n * q.rows[0] * q.rows[1] * q.rows[2]
            if kern in (E.IK["REG"], E.IK["DMA"], E.IK["P8"], E.IK["HALO"]) and hip.conv_igemm_mtiles(q) != -(-m // bm):
                bad.append((c.name, "mtiles", hip.conv_igemm_mtiles(q), m, bm))
        elif c.method == "conv_wgrad":
            r, ws, splits = hip.conv_wgrad_route(q)
            seen_w.add(r)
            if r != c.route or ws != c.ws or (c.many_splits is not None and (splits > 1) != c.many_splits):
                bad.append((c.name, E.route_name(c.route), c.ws, c.many_splits, E.route_name(r), ws, splits))
            if ws and hip.conv_wgrad_workspace_bytes(q) < 0:
                bad.append((c.name, "workspace bytes"))
    assert not bad, bad
    # per dtype: bit 28 of a route is the map dtype, so equality of the sets is equality per dtype
    assert seen_i == set(ig), ([ig[r] for r in set(ig) - seen_i], [hex(r) for r in seen_i - set(ig)])
    assert seen_w == set(wg), ([wg[r] for r in set(wg) - seen_w], [hex(r) for r in seen_w - set(wg)])


def test_route_query_returns_the_status_of_an_invalid_descriptor(hip):
    q, _ = _bound(E.BY_NAME["f32_reg128_last_row"], hip)
    from video_classification_amd._lib import SfkError
    bad = dataclasses.replace(q, cin=q.cin + 4)                  # cin != x.c: the library's validate() says SFK_ERR_INVALID
    assert hip.lib.sfk_conv_igemm_route(C.byref(_lib._c_conv(bad))) == -1
    with pytest.raises(SfkError, match=r"sfk_conv_igemm_route: .*\(-1\)"):
        hip.conv_route(bad)
    w, _ = _bound(E.BY_NAME["wg_f32_32x32_one_pixel"], hip)
    badw = dataclasses.replace(w, cout=w.cout + 4)
    assert hip.lib.sfk_conv_wgrad_route(C.byref(hip._wgrad_desc(badw))) == -1
    with pytest.raises(SfkError, match=r"sfk_conv_wgrad_route: .*\(-1\)"):
        hip.conv_wgrad_route(badw)
    odd = dataclasses.replace(q, y=FMap(torch.zeros(q.y.buf.numel() + 1)[1:], q.y.n, q.y.t, q.y.h, q.y.w, q.y.c, q.y.ld, q.y.c_off))   # y 4 bytes off
    assert hip.lib.sfk_conv_igemm_route(C.byref(_lib._c_conv(odd))) == -2                                   # SFK_ERR_UNSUPPORTED


def test_a_too_small_workspace_reports_the_atomics_route(hip):
    for name in ("wg_f32_64x32_m65", "wg_bf16_dma128_small_ws"):
        q, _ = _bound(E.BY_NAME[name], hip)
        assert q.workspace is not None and q.workspace.numel() * 4 == hip.conv_wgrad_workspace_bytes(q) - 16
        assert hip.conv_wgrad_route(q)[1] is False
        full = dataclasses.replace(q, workspace=torch.zeros(hip.conv_wgrad_workspace_bytes(q) // 4))
        assert hip.conv_wgrad_route(full)[1] is True and hip.conv_wgrad_route(full)[0] == hip.conv_wgrad_route(q)[0]


@pytest.mark.parametrize("case", [c for c in E.CASES if not c.slow], ids=lambda c: c.name)
def test_the_reference_alone_is_inside_every_bound(case):
    be = E.EdgeEmu()
    _, sig = _bound(case, be)
    r = la.replay(sig, be, "cpu", seed=case.seed)
    # a condition on the inputs: a case that misses the cap gets another `seed` in the table (the GPU test uses the same one)
    assert r.ambiguous < AMB_CAP, r.ambiguous
    assert r.ok, (r.verdicts, r.untouched_bad)


def test_slow_cases_stay_at_the_thresholds_of_the_big_tiles():
    assert all(n in E.BY_NAME for n in E.SLOW_ON_CPU)
    assert all(("t256" in n) or ("p8" in n) or ("256x128" in n) for n in E.SLOW_ON_CPU)


def test_small_bf16_maps_are_judged_by_their_elements_only_below_2048():
    """the rule lives in ref64 (bn_ref64 and launch_audit.replay use it from there) and loosens nothing at 2048 elements"""
    import bn_ref64
    assert bn_ref64.SMALL_MAP == ref64.SMALL_MAP == 2048
    assert ref64.elem_only("map_bf16", 2047) and not ref64.elem_only("map_bf16", 2048)
    assert not ref64.elem_only("map_f32", 8) and not ref64.elem_only("sum_f32", 8)
    g = torch.Generator().manual_seed(0)
    r = torch.randn(24, generator=g, dtype=torch.float64)
    y = r * (1 + 1.15 * 2.0 ** -9)                           # every element half an ulp or so off: elements pass, the rms does not
    v, w = ref64.compare("m", y, r, r.abs(), 8, torch.bfloat16, "map_bf16"), ref64.judge("m", y, r, r.abs(), 8, torch.bfloat16, "map_bf16")
    assert v.worst <= 1.0 and not v.ok and w.ok
    assert not ref64.judge("m", r * 1.5, r, r.abs(), 8, torch.bfloat16, "map_bf16").ok
    big = torch.randn(4096, generator=g, dtype=torch.float64)
    assert not ref64.judge("m", big * (1 + 2.0 ** -8.5), big, big.abs(), 8, torch.bfloat16, "map_bf16").ok


def test_no_production_signature_has_a_bf16_map_below_2048_elements():
    """so the small-map rule (ref64.elem_only) that launch_audit.replay now applies loosens nothing in the production audit
    (tests/test_gpu_launch_audit.py): every bf16 map its plans bind -- input or output -- has 2048 elements or more"""
    from emu_stem2d import EmuStem2dBackend
    rec = la.record_plans(EmuStem2dBackend(), "cpu", la.PRODUCTION)
    assert len(rec.calls) > 500

    def maps(e, out):
        if isinstance(e, tuple) and e and e[0] == "F":
            out.append(e)
        elif isinstance(e, tuple):
            for x in e:
                maps(x, out)
    small = []
    for sig in rec.calls:
        found = []
        maps(sig[1], found)
        small += [(la.describe(sig), e) for e in found if e[1] == "bf16" and e[2] * e[3] * e[4] * e[5] * e[6] < ref64.SMALL_MAP]
    assert not small, small[:3]


# ----------------------------------------------------------------------------- mutations
def _mutant(method, pre=None, snap=None, post=None):
    """an EdgeEmu whose `method` runs on pre(p) instead of p and / or has its outputs tampered with by post(p, snap(p))"""
    class M(E.EdgeEmu):
        pass

    def call(self, p):
        run = getattr(E.EdgeEmu, method)(self, pre(p) if pre else p)

        def r(stream):
            s = snap(p) if snap else None
            run(stream)
            if post:
                post(p, s)
        return r
    setattr(M, method, call)
    return M()


def _rows(f: FMap):
    return f.view5().reshape(-1, f.c)


def _shift_c_off(p):
    x = p.x
    return dataclasses.replace(p, x=FMap(x.buf, x.n, x.t, x.h, x.w, x.c, x.ld, x.c_off + 4))


def _drop_k_tail(p):
    w = p.w.clone()
    w[: p.cout * p.wtaps * p.cin].view(p.cout, p.wtaps, p.cin)[:, :, -1] = 0
    return dataclasses.replace(p, w=w)


def _one_pixel_past_m(p, _):
    mt = E.EdgeEmu().conv_igemm_mtiles(p)
    st = p.stats[: mt * p.cout * 2].view(mt, p.cout, 2)
    last = _rows(p.y)[-1].float()
    st[mt - 1, :, 0] += last
    st[mt - 1, :, 1] += last * last


def _flip_last_group_bit(p, _):
    groups = p.cout // (8 if p.y.dtype == torch.bfloat16 else 4)
    p.ep.relu_bits[groups - 1] ^= 1


def _lose_a_split(p, _):
    X, D = _rows(p.x).float(), _rows(p.dy).float()
    p.dw[: p.cout * p.wtaps * p.cin].view(p.cout, p.wtaps, p.cin)[:, 0, :] -= D[64:128].t() @ X[64:128]


def _past_the_slice(p, _):
    y = p.dg_y
    y.buf[y.c_off + y.c + (y.ld - y.c_off - y.c)] = 7.0            # first element behind pixel 0's record: pixel 1, channel 0


MUTATIONS = {
    "last row of a ragged tile dropped": ("f32_reg128_last_row", "conv_igemm", dict(
        snap=lambda p: _rows(p.y)[-1].clone(), post=lambda p, s: _rows(p.y)[-1].copy_(s))),
    "last row duplicated from the previous row": ("bf16_dma128_wide_last_row", "conv_igemm", dict(
        post=lambda p, s: _rows(p.y)[-1].copy_(_rows(p.y)[-2]))),
    "partial-sum row includes a pixel past M": ("bf16_dma128_wide_last_row", "conv_igemm", dict(post=_one_pixel_past_m)),
    "c_off off by 4": ("f32_reg128_last_row", "conv_igemm", dict(pre=_shift_c_off)),
    "K-tail channel dropped": ("bf16_reg16_short_12ch_acc", "conv_igemm", dict(pre=_drop_k_tail)),
    "oo off by one in a strided pass": ("f32_reg64_dgrad_s2_pass1", "conv_igemm", dict(
        pre=lambda p: dataclasses.replace(p, oo=(0, 0, 0)))),
    "old values ignored in a += pass": ("bf16_dma128_dgrad_s2_pass3", "conv_igemm", dict(
        pre=lambda p: dataclasses.replace(p, accumulate=False))),
    "res_shift dropped": ("bf16_dma128_ep_res", "conv_igemm", dict(
        pre=lambda p: dataclasses.replace(p, ep=dataclasses.replace(p.ep, res_shift=None)))),
    "bitmap byte of the last channel group wrong": ("f32_reg128_ep_all", "conv_igemm", dict(post=_flip_last_group_bit)),
    "unlisted dw tap overwritten": ("wg_f32_32x32_m63_subset", "conv_wgrad", dict(
        post=lambda p, s: p.dw[: p.cout * p.wtaps * p.cin].view(p.cout, p.wtaps, p.cin)[:, 1, :].zero_())),
    "one workspace split missing": ("wg_bf16_128x32_many", "conv_wgrad", dict(post=_lose_a_split)),
    "write one element past a sliced dg_y": ("wg_bf16_dma256_dg_slice", "conv_wgrad", dict(post=_past_the_slice)),
}


@pytest.mark.parametrize("what", list(MUTATIONS), ids=lambda s: s.replace(" ", "_"))
def test_replay_refuses_the_mutation(what):
    name, method, how = MUTATIONS[what]
    case = E.BY_NAME[name]
    assert case.method == method
    _, sig = _bound(case, E.EdgeEmu())
    assert la.replay(sig, E.EdgeEmu(), "cpu", seed=case.seed).ok
    r = la.replay(sig, _mutant(method, **how), "cpu", seed=case.seed)
    assert not r.ok, (what, r.verdicts)
