"""Every conv / filter-gradient route of include/sfk.h at its tile edges, on the GPU (the table: tests/conv_edges.py).
Each case is recorded through launch_audit.Recorder(HipBackend()), must report the route it declares -- a retune that moves a
test shape to another kernel FAILS here instead of covering less --, is launched ONCE by launch_audit.replay on seeded,
guarded buffers and held to ref64.compare per element (the references are float64 matmuls on the device) with every byte
outside the written region unchanged.  Workspace routes of the filter gradient run a second time and must repeat dw bit for
bit.  One line per case; the worst figures per route and the wall time are printed at the end."""
import collections
import ctypes as C
import time

import pytest
import torch

import conv_edges as E
import launch_audit as la

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WORST = collections.defaultdict(lambda: [0.0, 0.0, 0])          # route name -> [worst error / bound, agg / bound, cases]
T0 = [None, 0.0]
AMB_CAP = 1e-3            # share of ambiguous ReLU signs a case may excuse (bn_ref64.AMB_CAP)


def _default_tuning() -> bool:
    from video_classification_amd import _lib
    lib, t, d = _lib.load(), _lib.tuning(), _lib.new_tuning()
    assert lib.sfk_default_tuning(C.byref(d)) == 0
    return all(getattr(t, f) == getattr(d, f) for f, _ in _lib._Tuning._fields_)


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    if not _default_tuning():
        pytest.skip("the route declarations of tests/conv_edges.py hold for the default tuning table only")
    T0[0] = time.time()
    return HipBackend()


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.name)
def test_case_reaches_its_route_and_matches_float64(hip, case):
    t1 = time.time()
    rec = la.Recorder(hip)
    q = case.bind(rec, DEV)
    (sig,) = rec.calls
    if case.method == "conv_igemm":
        bound_route = hip.conv_route(q)
        assert bound_route == case.route, (E.route_name(case.route), E.route_name(bound_route))
    elif case.method == "conv_wgrad":
        bound_route, ws, splits = hip.conv_wgrad_route(q)
        assert (bound_route, ws) == (case.route, case.ws), (E.route_name(case.route), case.ws, E.route_name(bound_route), ws)
        assert case.many_splits is None or (splits > 1) == case.many_splits, splits
    del q, rec
    r = la.replay(sig, hip, DEV, seed=case.seed)
    tag = case.method if case.route is None else E.route_name(case.route)
    if case.method == "conv_igemm":
        assert r.route == case.route, (E.route_name(case.route), E.route_name(r.route))
    elif case.method == "conv_wgrad":
        assert r.route[:2] == (case.route, case.ws), r.route
        tag += f" ws={int(r.route[1])} splits={r.route[2]}"
    repeat = ""
    if case.method == "conv_wgrad" and case.ws:
        dw1 = r.args["p"].dw.clone()
        dw2 = la.replay(sig, hip, DEV, seed=case.seed).args["p"].dw
        assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)), "the workspace path did not repeat dw bit for bit"
        repeat = " repeat bit-equal"
    w = WORST[tag.split(" ")[0]]
    w[0], w[1], w[2] = max(w[0], r.worst), max(w[1], r.agg), w[2] + 1
    dt = time.time() - t1
    T0[1] += dt
    print(f"\n{'ok  ' if r.ok else 'FAIL'} {case.name}: {tag} worst {r.worst:.3g} agg/bound {r.agg:.3g} ambiguous {r.ambiguous:.2g}{repeat} {dt:.2f} s"
          + ("" if r.ok else f" {r.verdicts} untouched-bad {r.untouched_bad}"))
    assert r.ok, (r.verdicts, r.untouched_bad)
    assert r.ambiguous < AMB_CAP, r.ambiguous         # (the seed is the table's, as on the CPU: nothing is reseeded here)
    torch.cuda.empty_cache()


def test_zz_worst_per_route(hip):
    """(runs last) the summary table: route, cases, worst error / bound, worst aggregate / bound"""
    print()
    for name in sorted(WORST):
        w = WORST[name]
        print(f"  {name}: {w[2]} cases, worst error/bound {w[0]:.3g}, aggregate/bound {w[1]:.3g}")
    print(f"  {sum(w[2] for w in WORST.values())} cases in {T0[1]:.1f} s of case time, {time.time() - T0[0]:.1f} s wall")
