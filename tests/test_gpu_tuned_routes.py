"""The kernels only a non-default sfk_tuning table reaches, on the GPU (the tables and cases: tests/tuned_tables.py).  The table
is write-once per process, so each table runs in a fresh child (tests/tuned_worker.py TABLE gpu OUT), one at a time, started
by the first test that needs it; the child binds every case, replays ONCE each case the table moves or adds (launch_audit.replay
on seeded, guarded buffers, held to ref64.compare per element; under `alt` also the BatchNorm tables and the pooling cases
through bn_ref64.check_*) and writes one JSON line per case.  A test here reads its case's line and asserts the declared route
(of the bound AND of the replayed descriptor), every verdict inside its bound, every byte outside the written region unchanged,
the ambiguous-sign share under the cap, dw bit-equal on a second replay where the workspace path ran, and -- where the line
lists BatchNorm launches -- the partial rows and the cache-hint instantiation restated from the header's rules.
A child that ends by a signal, an abort, a non-zero exit (the worker's answer to the first HIP error) or its time limit is
recorded: its tests fail, and no later table's child is started -- after a fault nothing more goes to the GPU."""
import os
import subprocess
import time

import pytest

import bn_ref64 as B
import conv_edges as E
import stem_edges as S
import tuned_tables as T
from test_tuned_routes_cpu import read_lines, run_worker

pytestmark = pytest.mark.gpu
AMB_CAP = 1e-3            # share of ambiguous ReLU signs a case may excuse (bn_ref64.AMB_CAP)
TABLES = list(T.TABLES)
# seconds a child may take: three times its measured wall time on an MI355X (torch import and HIP initialisation vary with the
# machine's load).  Measured, process start to exit: narrow 2.9 s, alt 4.6 s, off 2.8 s as a file of
# its own (2.5 / 4.0 / 2.5 s inside the whole suite; about 1 / 2.7 / 0.7 s of that in the loop over the cases).
CHILD_LIMIT = {"narrow": 9, "alt": 14, "off": 9}


def _bn_lines():
    return ([f"bn_apply:{B.case_name(c)}" for c in B.APPLY_CASES + B.SUMS_CASES]
            + [f"bn_bwd_apply:{B.case_name(c)}" for c in B.BWD_APPLY_CASES] + [f"pool:{T.pool_name(c)}" for c, _, _ in T.POOL_CASES]
            + [f"head_pool:{c['name']}" for c, _, _ in T.HEAD_POOL_CASES])


def replayed(table: str):
    """the lines of the table's child that carry a replay"""
    names = T.moved(table) + [c.name for c in T.NEW[table]]
    if table in T.NT:
        names += [c.name for c in E.CASES if c.method in T.BN_METHODS] + _bn_lines()
    assert len(set(names)) == len(names)
    return names


class Children:
    def __init__(self, tmp):
        self.tmp, self.lines, self.failed, self.fault = tmp, {}, {}, None

    def get(self, table: str) -> dict:
        if table in self.failed:
            pytest.fail(self.failed[table])
        if table not in self.lines:
            if self.fault:
                self.failed[table] = f"not started: {self.fault}; nothing more goes to the GPU"
                pytest.fail(self.failed[table])
            path = str(self.tmp / f"{table}.jsonl")
            t0 = time.time()
            try:
                p = run_worker(table, "gpu", path, CHILD_LIMIT[table])
                how = None if p.returncode == 0 else f"exit status {p.returncode}: {p.stderr[-1500:]}"
            except subprocess.TimeoutExpired:
                how = f"no end within {CHILD_LIMIT[table]} s"
            lines = read_lines(path) if os.path.exists(path) else []
            if how is None and not (lines and lines[-1].get("done")):
                how = "no closing line"
            if how:
                last = lines[-1] if lines else None
                self.fault = self.failed[table] = f"the child of table {table} ended abnormally ({how}); its last line: {last}"
                pytest.fail(self.fault)
            print(f"\n  table {table}: {len(lines) - 1} lines, the child took {time.time() - t0:.1f} s from start to exit "
                  f"({lines[-1]['wall']} s in its loop over the cases); limit {CHILD_LIMIT[table]} s")
            self.lines[table] = {ln["case"]: ln for ln in lines[:-1]}
        return self.lines[table]


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    return Children(tmp_path_factory.mktemp("tuned_gpu"))


PARAMS = [(t, n) for t in TABLES for n in replayed(t)]


@pytest.mark.parametrize("table,name", PARAMS, ids=[f"{t}-{n}" for t, n in PARAMS])
def test_case_reaches_its_route_and_matches_float64(children, table, name):
    ln = children.get(table)[name]
    assert "error" not in ln, ln
    case = T.NEW_BY_NAME[table].get(name) or E.BY_NAME.get(name) or S.BY_NAME.get(name)
    if case is not None:
        assert not T.check_line(table, case, ln), T.check_line(table, case, ln)
        want = T.expected(table, case)
        if "route" in want:                                # ... and the descriptor that was LAUNCHED reports it too
            assert ln["replay_route"] == want["route"], (hex(ln["replay_route"]), hex(want["route"]))
        if case.method == "conv_wgrad":
            assert ln["replay_ws"] == want["ws"]
            if want["ws"]:
                assert ln["repeat_equal"] is True, "the workspace path did not repeat dw bit for bit"
        if isinstance(case, S.Case):
            assert (ln["replay_units"], ln["replay_grid"]) == (ln["units"], ln["grid"])
    print(f"\n{'ok  ' if ln['ok'] else 'FAIL'} {table} {name}: worst {ln['worst']:.3g} agg/bound {ln.get('agg', 0.0):.3g} "
          f"ambiguous {ln.get('ambiguous', 0.0):.2g} {ln['seconds']} s" + ("" if ln["ok"] else f" {ln['failed']}"))
    assert ln["ok"], ln["failed"]
    assert ln.get("untouched_ok", True)
    assert ln.get("ambiguous", 0.0) < AMB_CAP, ln["ambiguous"]
    bn_parts = T.TABLES[table].get("SFK_BN_PARTS", 1024)
    for b in ln.get("launches", ()):
        if b["nparts"] is not None:
            assert b["nparts"] == T.nparts_rule(b["cgs"], b["pixels"], b["max_parts"] or 0, bn_parts), b
        if b["method"] in T.NT_FIELD:                       # which instantiation the case took, from the header's threshold rule
            mb = T.TABLES[table][{"nt_apply_mb": "SFK_NT_APPLY_MB", "nt_reduce_mb": "SFK_NT_RED_MB",
                                  "nt_bwd_apply_mb": "SFK_NT_BAPP_MB"}[T.NT_FIELD[b["method"]]]]
            assert b["nt"] == T.nt_rule(b["bytes"], mb) == T.NT[table][b["method"]], b


def test_zz_worst_per_route(children):
    """(runs last) per table: route, cases, worst error / bound, worst aggregate / bound -- the rows of DESIGN.md 12e"""
    for table in TABLES:
        if table not in children.lines:
            continue
        rows = {}
        for ln in children.lines[table].values():
            if "worst" not in ln:
                continue
            r = ln.get("route")
            tag = ln["kind"] if r is None else (S.route_name(r) if ln["kind"].startswith("stem") else T.route_name(r))
            w = rows.setdefault(tag, [0.0, 0.0, 0, 0.0])
            w[0], w[1], w[2], w[3] = max(w[0], ln["worst"]), max(w[1], ln.get("agg", 0.0)), w[2] + 1, w[3] + ln["seconds"]
        print(f"\n  table {table}")
        for tag in sorted(rows):
            w = rows[tag]
            print(f"    {tag}: {w[2]} cases, worst error/bound {w[0]:.3g}, aggregate/bound {w[1]:.3g}, {w[3]:.1f} s")
