"""Every stem route of include/sfk.h at its tile, half-tile, pair and chunk edges, on the GPU (the table: tests/stem_edges.py).
Each case is recorded through launch_audit.Recorder(HipBackend()), must report the route (and, where it declares them, the
work items and workgroups) it declares -- a retune, or one alignment bit, that moves a test shape to another kernel FAILS here
instead of covering less --, is launched ONCE by launch_audit.replay on seeded, guarded buffers and held to ref64.compare per
element against the float64 restatement, with every byte outside the written region unchanged.  A case that declares a
refusal must return that status and write nothing.  The uint8 and pooled stems are held to the same restatement over the
materialised clip and, forward, to the bits of the float entry point on it.  One line per case; the worst figures per route
and the wall time are printed at the end."""
import collections
import ctypes as C
import time

import pytest
import torch

import launch_audit as la
import stem_edges as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WORST = collections.defaultdict(lambda: [0.0, 0.0, 0])          # route name -> [worst error / bound, agg / bound, cases]
T0 = [None, 0.0]


def _default_tuning() -> bool:
    from video_classification_amd import _lib
    lib, t, d = _lib.load(), _lib.tuning(), _lib.new_tuning()
    assert lib.sfk_default_tuning(C.byref(d)) == 0
    return all(getattr(t, f) == getattr(d, f) for f, _ in _lib._Tuning._fields_)


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    if not _default_tuning():
        pytest.skip("the route declarations of tests/stem_edges.py hold for the default tuning table only")
    T0[0] = time.time()
    return HipBackend()


def _guarded(fn, *a, **kw):
    """run one GPU step; a HIP error (a fault, not a mismatch) ends the session: nothing more is started on a faulted device"""
    try:
        return fn(*a, **kw)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"GPU fault, nothing more is run: {e}", returncode=3)
        raise


def _note(tag, r):
    w = WORST[tag]
    w[0], w[1], w[2] = max(w[0], r.worst), max(w[1], r.agg), w[2] + 1


def _routed(hip, case, p, m):
    """the route query on (p, m) against the case's declarations; the route's name"""
    if case.route is None:
        return case.method
    route, units, grid = hip.stem_route(p, m, E.is_wgrad(case.method))
    assert route == case.route, (E.route_name(case.route), E.route_name(route))
    assert case.units is None or units == case.units, (units, case.units)
    assert case.grid is None or grid == case.grid, (grid, case.grid)
    assert case.wrap is None or (units > grid) == case.wrap, (units, grid)
    return f"{E.route_name(route)} items={units} grid={grid}"


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.name)
def test_case_reaches_its_route_and_matches_float64(hip, case):
    t1 = time.time()
    p, m, sig = E.bound(case, hip, DEV)
    if case.status < 0:
        if not case.method.startswith("stem2d"):
            with pytest.raises(Exception, match=rf"\({case.status}\)"):
                hip.stem_route(p, m, E.is_wgrad(case.method))
        del p, m
        status, untouched = _guarded(E.replay_refused, sig, hip, DEV, case.seed)
        print(f"\n{'ok  ' if (status, untouched) == (case.status, True) else 'FAIL'} {case.name}: refused with {status}, "
              f"buffers {'untouched' if untouched else 'WRITTEN'}")
        assert status == case.status and untouched
        return
    _routed(hip, case, p, m)
    del p, m
    r = _guarded(la.replay, sig, hip, DEV, seed=case.seed)
    tag = _routed(hip, case, r.args["p"], r.args["dy" if E.is_wgrad(case.method) else "y"])       # the REPLAYED descriptor's
    spread = ""
    if case.twice:                   # atomics: the sums need not repeat bit for bit; both runs are held to float64
        r2 = _guarded(la.replay, sig, hip, DEV, seed=case.seed)
        d = (r.args["dw"].double() - r2.args["dw"].double()).abs().max()
        spread = f" second run worst {r2.worst:.3g}, max |dw1 - dw2| {float(d):.3g} (max |dw| {float(r.args['dw'].abs().max()):.3g})"
        assert r2.ok, (r2.verdicts, r2.untouched_bad)
    _note(tag.split(" ")[0], r)
    dt = time.time() - t1
    T0[1] += dt
    print(f"\n{'ok  ' if r.ok else 'FAIL'} {case.name}: {tag} worst {r.worst:.3g} agg/bound {r.agg:.3g}{spread} {dt:.2f} s"
          + ("" if r.ok else f" {r.verdicts} untouched-bad {r.untouched_bad}"))
    assert r.ok, (r.verdicts, r.untouched_bad)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", E.U8, ids=lambda c: c.name)
def test_u8_case_matches_float64_and_the_float_entry_point(hip, case):
    t1 = time.time()
    r, same = _guarded(E.u8_run, case, hip, DEV, float_be=hip)
    _note(f"{case.method}<{case.tag}>", r)
    dt = time.time() - t1
    T0[1] += dt
    print(f"\n{'ok  ' if r.ok and same is not False else 'FAIL'} {case.name}: {case.method}<{case.tag}> worst {r.worst:.3g} "
          f"agg/bound {r.agg:.3g}{'' if same is None else ' bits of the float entry point: ' + str(same)} {dt:.2f} s"
          + ("" if r.ok else f" {r.verdicts} untouched-bad {r.untouched_bad}"))
    assert r.ok, (r.verdicts, r.untouched_bad)
    assert same is not False, "the uint8 stem's map / statistics differ from the float entry point's on the materialised clip"
    torch.cuda.empty_cache()


def test_zz_worst_per_route(hip):
    """(runs last) the summary table: route, cases, worst error / bound, worst aggregate / bound"""
    print()
    for name in sorted(WORST):
        w = WORST[name]
        print(f"  {name}: {w[2]} cases, worst error/bound {w[0]:.3g}, aggregate/bound {w[1]:.3g}")
    print(f"  {sum(w[2] for w in WORST.values())} cases in {T0[1]:.1f} s of case time, {time.time() - T0[0]:.1f} s wall")
