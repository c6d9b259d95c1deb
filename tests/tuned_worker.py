"""TEST INFRASTRUCTURE: one tuning table of tests/tuned_tables.py in a process of its own (the table is write-once per
process).  Run only as a child, with the table's environment set by the parent:

    python tests/tuned_worker.py TABLE MODE OUT         TABLE narrow | alt | off (default: the baseline of the pins)

It first asserts that the loaded library's table is the default one with exactly the table's fields replaced, so a
misspelt knob cannot quietly run the defaults.  MODE routes needs no GPU: every case of conv_edges / stem_edges and every
new case of the table is bound on CPU tensors and what the library's route queries report is written to OUT, one JSON line
per case.  MODE gpu does the same on the device and then replays, once, every case the table moves or adds (and, where the
table declares cache hints, the BatchNorm tables of bn_ref64 and the pooling cases) through launch_audit.replay /
bn_ref64.check_* as they stand, one JSON line per case: worst error / bound, aggregate / bound, ambiguous share, untouched
bytes, the route of the replayed descriptor.  The first exception out of a launch or a synchronize ends the process: what it
has is written, it exits non-zero and launches nothing more."""
import ctypes as C
import functools
import inspect
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import bn_ref64 as B  # noqa: E402
import conv_edges as E  # noqa: E402
import head_ref64 as H  # noqa: E402
import launch_audit as la  # noqa: E402
import stem_edges as S  # noqa: E402
import tuned_tables as T  # noqa: E402
from video_classification_amd import _lib  # noqa: E402
from video_classification_amd._lib import HipBackend, SfkError  # noqa: E402


def check_table(table: str):
    """the library runs the default table with exactly the table's fields replaced"""
    want = {_lib.TUNING_ENV[k]: int(v) for k, v in T.env_of(table).items()}        # KeyError: no such knob
    stray = [k for k in _lib.TUNING_ENV if k in os.environ and k not in T.env_of(table)]
    assert not stray, f"knobs outside the table are set: {stray}"
    lib, got, dflt = _lib.load(), _lib.tuning(), _lib.new_tuning()
    assert lib.sfk_default_tuning(C.byref(dflt)) == 0
    for f, _ in _lib._Tuning._fields_:
        w = want.get(f, getattr(dflt, f))
        assert getattr(got, f) == w, f"sfk_tuning.{f} is {getattr(got, f)}, the table says {w}"
    for f, v in want.items():
        assert v != getattr(dflt, f), f"{f} = {v} is the default: the table would test nothing with it"


class Spy(HipBackend):
    """HipBackend that notes, for every BatchNorm launch it binds, the map's geometry and the partial rows reported"""
    NOTED = {"bn_stats": "y", "bn_apply": "y", "bn_bwd_reduce": "da", "bn_bwd_apply": "y", "bn_maxpool_bwd_reduce": "y"}

    def __init__(self):
        super().__init__()
        self.seen = []

    def __getattribute__(self, name):
        attr = super().__getattribute__(name)
        if name not in Spy.NOTED:
            return attr

        @functools.wraps(attr)           # (launch_audit.Recorder reads the signature through __wrapped__)
        def noted(*a, **kw):
            res = attr(*a, **kw)
            b = inspect.signature(attr).bind(*a, **kw)
            b.apply_defaults()
            m = b.arguments[Spy.NOTED[name]]
            vec = 8 if m.dtype == torch.bfloat16 else 4
            mp = b.arguments.get("max_parts")
            if name == "bn_apply" and b.arguments.get("out_sums") is None:
                mp = None
            self.seen.append({"method": name, "cgs": m.c // vec, "pixels": m.pixels, "max_parts": mp,
                              "nparts": res[1] if isinstance(res, tuple) else None,
                              "bytes": m.pixels * m.c * (2 if m.dtype == torch.bfloat16 else 4)})
            return res
        return noted

    def drain(self):
        tn = _lib.tuning()
        out, self.seen = self.seen, []
        for s in out:
            f = T.NT_FIELD.get(s["method"])
            s["nt"] = None if f is None else T.nt_rule(s["bytes"], int(getattr(tn, f)))
        return out


def conv_report(hip, case, q) -> dict:
    if case.method == "conv_igemm":
        return {"route": hip.conv_route(q), "mtiles": hip.conv_igemm_mtiles(q), "family": hip.conv_family(q),
                "m": q.x.n * q.rows[0] * q.rows[1] * q.rows[2]}
    if case.method == "conv_wgrad":
        r, ws, splits = hip.conv_wgrad_route(q)
        return {"route": r, "ws": ws, "splits": splits, "m": q.dy.pixels}
    return {}


def stem_report(hip, case, p, m) -> dict:
    if case.method.startswith("stem2d"):         # one instantiation per dtype pair, no route query
        return {}
    try:
        r, units, grid = hip.stem_route(p, m, S.is_wgrad(case.method))
    except SfkError as e:
        return {"status": int(str(e).rsplit("(", 1)[1].rstrip(") "))}
    return {"status": 0, "route": r, "units": units, "grid": grid}


def replay_line(r: la.Replay) -> dict:
    return {"ok": bool(r.ok), "worst": r.worst, "agg": r.agg, "ambiguous": r.ambiguous, "untouched_ok": bool(r.untouched_ok),
            "failed": [str(v) for v in r.verdicts if not v.ok][:4], "verdicts": len(r.verdicts)}


def table_line(vs) -> dict:
    return {"ok": not B.failures(vs), "worst": B.worst_of(vs), "failed": [str(v) for v in B.failures(vs)][:4], "verdicts": len(vs)}


def main(argv) -> int:
    table, mode, out_path = argv
    assert mode in ("routes", "gpu") and (table == T.DEFAULT or table in T.TABLES)
    check_table(table)
    gpu = mode == "gpu"
    dev = torch.device("cuda", 0) if gpu else "cpu"
    hip = Spy()
    t0 = time.time()
    out = open(out_path, "w")
    state = {"case": None}

    def emit(d):
        out.write(json.dumps(d) + "\n")
        out.flush()

    replayed = set(T.moved(table)) | set(T.NEW_BY_NAME.get(table, {})) if table != T.DEFAULT else set()
    try:
        for case in T.conv_cases(table):
            state["case"] = case.name
            t1 = time.time()
            rec = la.Recorder(hip)
            q = case.bind(rec, dev)
            (sig,) = rec.calls
            line = {"case": case.name, "kind": case.method, **(conv_report(hip, case, q) if q is not None else {})}
            del q, rec
            bound = hip.drain()
            if bound:
                line["bound"] = bound                  # the partial rows the binding reports for the BatchNorm reductions
            if gpu and (case.name in replayed or (table in T.NT and case.method in T.BN_METHODS)):
                r = la.replay(sig, hip, dev, seed=case.seed)
                line.update(replay_line(r))
                line["launches"] = hip.drain()
                if case.method == "conv_igemm":
                    line["replay_route"] = r.route
                elif case.method == "conv_wgrad":
                    line["replay_route"], line["replay_ws"], line["replay_splits"] = r.route[0], bool(r.route[1]), r.route[2]
                    if r.route[1]:
                        dw1 = r.args["p"].dw.clone()
                        dw2 = la.replay(sig, hip, dev, seed=case.seed).args["p"].dw
                        line["repeat_equal"] = bool(torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)))
                        del dw1, dw2
                del r
                torch.cuda.empty_cache()
                line["seconds"] = round(time.time() - t1, 3)
            emit(line)
        for case in S.CASES:
            state["case"] = case.name
            t1 = time.time()
            p, m, sig = S.bound(case, hip, dev)
            line = {"case": case.name, "kind": case.method, **stem_report(hip, case, p, m)}
            del p, m
            if gpu and case.name in replayed:
                r = la.replay(sig, hip, dev, seed=case.seed)
                line.update(replay_line(r))
                rr = stem_report(hip, case, r.args["p"], r.args["dy" if S.is_wgrad(case.method) else "y"])
                line["replay_route"], line["replay_units"], line["replay_grid"] = rr.get("route"), rr.get("units"), rr.get("grid")
                del r
                torch.cuda.empty_cache()
                line["seconds"] = round(time.time() - t1, 3)
            emit(line)
        if gpu and table in T.NT:
            hip.drain()
            tables = ([("bn_apply", c, B.check_apply, B.case_name(c)) for c in B.APPLY_CASES + B.SUMS_CASES]
                      + [("bn_bwd_apply", c, B.check_bwd_apply, B.case_name(c)) for c in B.BWD_APPLY_CASES]
                      + [("pool", c, B.check_pool, T.pool_name(c)) for c, _, _ in T.POOL_CASES]
                      + [("head_pool", c, H.check_pool, c["name"]) for c, _, _ in T.HEAD_POOL_CASES])
            for kind, c, check, name in tables:
                state["case"] = f"{kind}:{name}"
                t1 = time.time()
                vs = check(hip, dev, c)
                emit({"case": state["case"], "kind": kind, **table_line(vs), "launches": hip.drain(),
                      "seconds": round(time.time() - t1, 3)})
    except Exception as e:          # a HIP error, a refused launch, a failed synchronize: nothing more goes to the device
        emit({"case": state["case"], "error": f"{type(e).__name__}: {e}"[:2000]})
        out.close()
        return 3
    emit({"done": True, "table": table, "mode": mode, "wall": round(time.time() - t0, 2)})
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
