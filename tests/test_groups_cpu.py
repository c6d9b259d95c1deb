"""Parameter groups and frozen ranges without a GPU: Engine.param_segments on the mini SlowFast and on res2d, the contract of
include/sfk_groups.h on the emulated backend (tests/emu_groups.py) with every mutation rejected by the checks the GPU test runs
(tests/groups_ref.py), and the header's ABI and host-side rejections through the built library (they launch nothing)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import groups_ref as GR
import head_ref64 as H
import optim_ref64 as O
from emu_groups import EmuGroupsBackend
from emu_optim import EmuOptimBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
SMALL = O.COUNTS


def _mini(seed=0, backend=None):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=torch.float32, device="cpu", backend=backend or EmuGroupsBackend(), seed=seed)


def _res2d():
    from video_classification_amd.slowfast import resnet50_2d_engine
    return resnet50_2d_engine(num_class=7, clip_len=2, crop=64, dtype=torch.float32, device="cpu", backend=EmuGroupsBackend(),
                              depth=18)


def _batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 7, 4, 64, 64, generator=g), torch.randint(0, 7, (2,), generator=g)


# ------------------------------------------------------------------ Engine.param_segments
def _covered(segs):
    return sum(e - b for b, e, _, _ in segs)


@pytest.mark.parametrize("make", [_mini, _res2d], ids=["slowfast", "res2d"])
def test_param_segments_cover_the_arena_in_order_and_merge(make):
    eng = make().engine
    tensors = eng.param_tensors()
    assert tensors[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(tensors, tensors[1:]))
    assert tensors[-1][1] + tensors[-1][2] == eng.arena_numel                 # the padding travels with its tensor
    assert sorted(k for k, _, _ in tensors) == sorted(k for k, v in eng.state_dict().items()
                                                      if v.is_floating_point() and "running_" not in k and k not in eng.dead)
    assert eng.param_segments() == [(0, eng.fc_b_off, 0, 1), (eng.fc_b_off, eng.arena_numel, 0, 0)]
    assert eng.param_segments(decay_scope="all") == [(0, eng.arena_numel, 0, 1)]
    first = tensors[0][0]
    prefix = first.split(".")[0] + "."
    segs = eng.param_segments([prefix], (), "weights")
    assert all(a[1] <= b[0] for a, b in zip(segs, segs[1:])) and _covered(segs) == eng.arena_numel
    assert all((a[1] < b[0]) or (a[2:] != b[2:]) for a, b in zip(segs, segs[1:])), "adjacent equal ranges did not merge"
    in_group = sum(n for k, _, n in tensors if k.startswith(prefix))
    assert sum(e - b for b, e, g, _ in segs if g == 1) == in_group > 0
    assert all(d == (1 if b < eng.fc_b_off else 0) for b, _, _, d in segs)
    frozen = eng.param_segments((), [prefix])
    assert _covered(frozen) == eng.arena_numel - in_group and all(g == 0 for _, _, g, _ in frozen)
    with pytest.raises(ValueError, match="matches no key"):
        eng.param_segments(["no.such.prefix."])
    with pytest.raises(ValueError, match="matches no key"):
        eng.param_segments((), ["blocks.9."])
    with pytest.raises(ValueError):
        eng.param_segments(["@stale"])
    with pytest.raises(ValueError):
        eng.param_segments(decay_scope="bias")


def test_first_matching_selector_wins_and_freeze_beats_groups():
    eng = _mini().engine
    t = {k: (off, n) for k, off, n in eng.param_tensors()}
    k = "blocks.1.multipathway_blocks.0.res_blocks.0.branch2.conv_a.weight"
    a = eng.param_segments(["blocks.1.multipathway_blocks.0.", "blocks.1."])
    b = eng.param_segments(["blocks.1.", "blocks.1.multipathway_blocks.0."])
    grp = lambda segs, off: next(g for s, e, g, _ in segs if s <= off < e)
    assert grp(a, t[k][0]) == 1 and grp(b, t[k][0]) == 1
    fast = "blocks.1.multipathway_blocks.1.res_blocks.0.branch2.conv_a.weight"
    assert grp(a, t[fast][0]) == 2 and grp(b, t[fast][0]) == 1
    assert not any(g == 2 for _, _, g, _ in b)
    c = eng.param_segments(["blocks.1."], ["blocks.1.multipathway_blocks.0."])
    assert not any(s <= t[k][0] < e for s, e, _, _ in c) and grp(c, t[fast][0]) == 1
    assert eng.frozen_param_keys(["blocks.6."]) == {"blocks.6.proj.weight", "blocks.6.proj.bias"}


def test_fresh_and_pretrained_resolve_against_the_load(tmp_path):
    """a synthetic 'pretrained' state dict with the 12 mismatching tensors removed, through ModelManager.load_pretrained"""
    from video_classification_amd.config import get_cfg
    from video_classification_amd.train import ModelManager
    m = _mini(seed=3)
    eng = m.engine
    assert eng.fresh_keys is None
    allp = [k for k, _, _ in eng.param_tensors()]
    assert _covered(eng.param_segments((), ["@fresh"])) == 0                     # nothing loaded: every key is fresh
    assert _covered(eng.param_segments((), ["@pretrained"])) == eng.arena_numel
    state = {k: v + 1 if v.is_floating_point() else v for k, v in _mini(seed=4).state_dict().items()}
    state["blocks.6.proj.weight"], state["blocks.6.proj.bias"] = torch.zeros(400, 10), torch.zeros(400)   # delete_mismatch wants them
    n0 = len(state)
    state = ModelManager.delete_mismatch(state)
    assert n0 - len(state) == 12
    cfg = get_cfg()
    cfg.MODEL.NAME = "slowfast-LHand"
    mm = ModelManager(cfg, device="cpu", backend=EmuGroupsBackend())
    mm.load_pretrained(m, state)
    fresh = {k for k in allp if k not in state}
    assert mm.fresh_keys >= fresh and eng.fresh_keys == mm.fresh_keys and len(fresh) == 12
    segs = eng.param_segments((), ["@pretrained"])
    t = {k: (off, n) for k, off, n in eng.param_tensors()}
    assert _covered(segs) == sum(t[k][1] for k in fresh)
    assert eng.frozen_param_keys(["@pretrained"]) == frozenset(allp) - fresh
    grp = eng.param_segments([("@pretrained")])
    assert sum(e - b for b, e, g, _ in grp if g == 0) == sum(t[k][1] for k in fresh)
    assert eng.frozen_param_keys(["@fresh"]) == frozenset(fresh)


# ------------------------------------------------------------------ the contract on the emulated backend, and its mutants
def _run_updates(be, count, ref64=False, pick=lambda name, kernel: True):
    vs = []
    for name, segs, kernel, off, sh, clip, mode, nesterov, momentum in GR.update_case_table(count):
        if pick(name, kernel):
            vs += GR.check_update_groups(be, EmuOptimBackend(), CPU, kernel, count, segs, 1, off, sh, clip, mode,
                                         nesterov=nesterov, momentum=momentum, ref64=ref64, tag=name)
    return vs


def _run_norms(be, count):
    vs = []
    for name, segs in GR.tables_for(count).items():
        for kind in ("randn", "nan_frozen", "inf_frozen", "nan", "inf"):
            vs += GR.check_norm_groups(be, EmuOptimBackend(), CPU, count, segs, kind, off=count % 2, tag=name)
    return vs


@pytest.mark.parametrize("count", SMALL)
def test_emu_groups_meet_the_contract(count):
    vs = _run_updates(EmuGroupsBackend(), count, ref64=count in (5, 1025)) + _run_norms(EmuGroupsBackend(), count)
    assert not H.failures(vs), H.failures(vs)[:5]


def test_case_tables_reach_what_the_issue_lists():
    segs = GR.tables_for(4099)
    cuts = {x for b, e, _, _ in segs["bounds"] for x in (b, e)}
    assert {0, 1, 3, 4, 5, 1023, 1024, 1025, 4098, 4099} <= cuts | {1025}
    assert segs["bounds"][0][0] == 0 and segs["bounds"][-1][1] == 4099
    assert 900 <= len(segs["many"]) <= 1100 and {g for _, _, g, _ in segs["many"]} == {0, 1, 2}
    runs = [e - b for b, e, _, _ in segs["alternating"]]
    assert set(runs) <= set(range(1, 8)) and len(set(runs)) >= 4
    big = GR.seg_many(O.BIG)
    assert big[-1][1] == O.BIG and len(big) <= 2048
    rows = {tuple(c[3:]) for n in SMALL for c in GR.update_case_table(n)}
    assert {r[0] for r in rows} == {0, 1} and {r[1] for r in rows} == {None, H.BF16, H.F32} and {r[2] for r in rows} == {False, True}
    assert {r[3] for r in rows} == set(O.MODES)


def _mutant(**attrs):
    return type("Mutant", (EmuGroupsBackend,), attrs)()


def _rejected(vs) -> bool:
    return bool(H.failures(vs))


@pytest.mark.parametrize("attr", ["visit_frozen", "skip_segment_last", "wrong_group_row", "ignore_decay_flag"])
@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_update_mutants_are_rejected(attr, kernel):
    be = _mutant(**{attr: True})
    hit = [count for count in SMALL if _rejected(_run_updates(be, count, pick=lambda n, k: k == kernel))]
    assert hit, f"{attr} passes every check of the {kernel} table"
    assert not _rejected(_run_updates(EmuGroupsBackend(), 1025, pick=lambda n, k: k == kernel))


def test_norm_over_frozen_ranges_is_rejected():
    be = _mutant(norm_over_frozen=True)
    assert all(_rejected(_run_norms(be, count)) for count in SMALL if count > 1)
    assert not _rejected(_run_norms(EmuGroupsBackend(), 1025))


def test_emu_rejects_what_the_host_rejects():
    be = EmuGroupsBackend()
    n = 64
    for segs in ([(8, 4, 0, 0)], [(0, 8, 0, 0), (4, 12, 0, 0)], [(16, 24, 0, 0), (0, 8, 0, 0)], [(0, n + 1, 0, 0)], [(-1, 4, 0, 0)],
                 [(0, 8, 3, 0)], [(0, 8, -1, 0)], [(4, 4, 0, 0)], [(i, i + 1, 0, 0) for i in range(2049)]):
        with pytest.raises(ValueError):
            be.group_table(segs, GR.WDS, max(n, 4096) if len(segs) > 100 else n)
    with pytest.raises(ValueError):
        be.group_table([], [0.0] * 65, n)
    with pytest.raises(ValueError):
        be.group_table([], [], n)


# ------------------------------------------------------------------ the ABI of include/sfk_groups.h
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from video_classification_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfk_groups.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_GROUPS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    assert lib.sfk_groups_abi_version() == _lib.GROUPS_ABI_VERSION == 1
    for n in ("group_table", "adam_groups", "sgd_groups", "grad_norm_groups"):
        assert callable(getattr(_lib.HipBackend, n))
    assert "optim_groups.hip" in open(os.path.join(ROOT, "video-classification_amd", "build.py")).read()


def test_struct_sizes_and_constants_match_the_header(lib, tmp_path):
    from video_classification_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_groups.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(sfk_group_seg), offsetof(sfk_group_seg, group), '
                   'sizeof(sfk_groups_hp), offsetof(sfk_groups_hp, nsegs), offsetof(sfk_groups_hp, lr_rows), '
                   'offsetof(sfk_groups_hp, clip_coef), SFK_GROUPS_MAX_SEGS, SFK_GROUPS_MAX_GROUPS, SFK_GROUPS_TILE);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)   # plain C, no HIP
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S, G = _lib._GroupSeg, _lib._GroupsHp
    assert out[:6] == [ctypes.sizeof(S), S.group.offset, ctypes.sizeof(G), G.nsegs.offset, G.lr_rows.offset, G.clip_coef.offset]
    assert out[6:] == [_lib.GROUPS_MAX_SEGS, _lib.GROUPS_MAX_GROUPS, 1024]


def _host_table(_lib, segs):
    arr = (_lib._GroupSeg * max(len(segs), 1))()
    for k, (b, e, g, d) in enumerate(segs):
        arr[k] = _lib._GroupSeg(b, e, 0, g, d)
    return arr


def test_prepare_numbers_the_tiles(lib):
    from video_classification_amd import _lib
    segs = [(0, 1, 0, 1), (1, 1024, 1, 0), (1024, 1025, 2, 0), (1030, 4099, 0, 1)]
    arr = _host_table(_lib, segs)
    assert lib.sfk_groups_prepare(ctypes.addressof(arr), 4, 4099, 3) == 1 + 1 + 1 + 4
    assert [arr[k].tile0 for k in range(4)] == [0, 1, 2, 3]
    assert lib.sfk_groups_prepare(None, 0, 4099, 1) == 0


def test_host_side_rejections_launch_nothing(lib):
    from video_classification_amd import _lib
    n = 4096
    p, step = torch.zeros(n), torch.zeros(1, dtype=torch.int64)
    rows, wds = torch.ones(3, 2), torch.zeros(3)
    P, S, B = p.data_ptr(), step.data_ptr(), ctypes.byref
    good = [(0, 5, 0, 1), (5, 1030, 1, 0), (2000, n, 2, 1)]

    def hp(table=good, prepare=True, **kw):
        arr = _host_table(_lib, table)
        if prepare:
            assert lib.sfk_groups_prepare(ctypes.addressof(arr), len(table), n, 3) >= 0
        d = _lib._GroupsHp()
        d.struct_size, d.decay_mode = ctypes.sizeof(_lib._GroupsHp), 1
        d.segs = d.segs_host = ctypes.addressof(arr)            # (the device copy is never read on the host)
        d.nsegs, d.ngroups, d.lr_rows, d.lr_len, d.weight_decay = len(table), 3, rows.data_ptr(), 2, wds.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        d._keep = arr
        return d
    adam = lambda d, count=n: lib.sfk_adam_groups(P, P, P, P, count, B(d) if d is not None else None, 0.9, 0.999, 1e-8, 1.0, S, None, 0, None)
    sgd = lambda d, count=n: lib.sfk_sgd_groups(P, P, P, count, B(d) if d is not None else None, 0.9, 0.0, 0, 1.0, S, None, 0, None)

    def raw(segs):       # a table the prepare step would refuse: tile0 filled by hand where that is not what is wrong
        return hp(segs, prepare=False)
    bad_tables = [[(5, 1030, 1, 0), (0, 5, 0, 1)], [(0, 8, 0, 0), (4, 12, 0, 0)], [(0, n + 1, 0, 0)], [(-4, 4, 0, 0)], [(8, 8, 0, 0)],
                  [(8, 4, 0, 0)], [(0, 8, 3, 0)], [(0, 8, -1, 0)]]
    for segs in bad_tables:
        arr = _host_table(_lib, segs)
        assert lib.sfk_groups_prepare(ctypes.addressof(arr), len(segs), n, 3) == -1, segs
        assert adam(raw(segs)) == -1 and sgd(raw(segs)) == -1, segs
        parts = torch.zeros(4, dtype=torch.float64)
        if segs[0][2] in (0, 1):       # (the norm does not read the group index)
            assert lib.sfk_grad_norm_groups(P, n, ctypes.addressof(arr), ctypes.addressof(arr), len(segs), 1.0, 1.0,
                                            parts.data_ptr(), P, None) == -1, segs
    stale = hp()
    stale._keep[2].tile0 += 1                                   # a tile0 that is not the prefix
    bad = [stale, hp(lr_rows=None), hp(weight_decay=None), hp(lr_len=0), hp(lr_len=-2), hp(segs=None), hp(segs_host=None),
           hp(nsegs=-1), hp(nsegs=2049), hp(ngroups=0), hp(ngroups=65), hp(ngroups=2), hp(decay_mode=3), hp(decay_mode=-1),
           hp(struct_size=0), hp(struct_size=ctypes.sizeof(_lib._GroupsHp) + 8), None]
    for i, d in enumerate(bad):
        assert adam(d) == -1 and sgd(d) == -1, i
    assert sgd(hp(decay_mode=2)) == -1                          # torch has no decoupled SGD
    assert adam(hp(), 0) == -1 and sgd(hp(), 0) == -1 and adam(hp(), 2048) == -1       # a segment past count
    huge = 1 << 42                                              # more (segment, tile) pairs than a grid has workgroups
    arr = _host_table(_lib, [(0, huge, 0, 1)])
    assert lib.sfk_groups_prepare(ctypes.addressof(arr), 1, huge, 3) == huge >> 10
    d = hp()
    d.segs = d.segs_host = ctypes.addressof(arr)
    d.nsegs = 1
    assert adam(d, huge) == -1 and sgd(d, huge) == -1
    assert lib.sfk_adam_groups(None, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, S, None, 0, None) == -1
    assert lib.sfk_adam_groups(P, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, None, None, 0, None) == -1
    assert lib.sfk_adam_groups(P, P, P, P, n, B(hp()), 0.9, 0.999, 1e-8, 1.0, S, P, 5, None) == -1
    assert lib.sfk_sgd_groups(P, P, None, n, B(hp()), 0.9, 0.0, 0, 1.0, S, None, 0, None) == -1      # momentum needs a buffer
    many = [(2 * i, 2 * i + 1, 0, 0) for i in range(2049)]
    arr = _host_table(_lib, many)
    assert lib.sfk_groups_prepare(ctypes.addressof(arr), 2049, 8192, 1) == -1
    assert lib.sfk_groups_prepare(ctypes.addressof(arr), 2048, 8192, 0) == -1 and lib.sfk_groups_prepare(ctypes.addressof(arr), 2048, 0, 1) == -1
    assert lib.sfk_groups_prepare(None, 3, 8192, 1) == -1
    parts = torch.zeros(4, dtype=torch.float64)
    D, A = parts.data_ptr(), ctypes.addressof(hp()._keep)
    gn = lambda g=P, count=n, segs=A, host=A, nsegs=3, mx=1.0, parts_=D, out=P: lib.sfk_grad_norm_groups(
        g, count, segs, host, nsegs, 1.0, mx, parts_, out, None)
    keep = hp()
    A = ctypes.addressof(keep._keep)
    for kw in (dict(g=None), dict(count=0), dict(segs=None), dict(host=None), dict(nsegs=-1), dict(nsegs=2049), dict(mx=-1.0),
               dict(mx=float("nan")), dict(parts_=None), dict(out=None), dict(count=2048)):
        assert gn(**dict(dict(segs=A, host=A), **kw)) == -1, kw
    assert int(step[0]) == 0 and not p.any()
