"""The three non-default tuning tables of tests/tuned_tables.py without a GPU:
  * closure -- tests/tuned_worker.py runs once per table in `routes` mode (a child process each: the table is write-once per
    process); every case of conv_edges / stem_edges and every new case reports exactly what tuned_tables declares for the
    table, sfk_conv_igemm_mtiles agrees with the reported tile, the partial rows of the BatchNorm reductions follow the
    header's rule, and the routes reached over the three tables, minus the default lists of include/sfk.h, are exactly its
    two SFK_*_ROUTES_TUNED lists;
  * the two ring depths and the two pointwise instantiations report different routes;
  * the reference alone -- every new case replayed on the torch restatement (EmuBackend) is inside every bound, so a GPU
    failure of a case is the kernel's;
  * mutations -- the ways the newly reached code goes wrong, each played on the emulated result, each refused."""
import dataclasses
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import bn_ref64 as B
import conv_edges as E
import head_ref64 as H
import launch_audit as la
import stem_edges as S
import tuned_tables as T
from emu_backend import EmuBackend
from test_conv_edges_cpu import _mutant as conv_mutant, _rows
from test_stem_edges_cpu import _mutant as stem_mutant
from video_classification_amd import _lib

AMB_CAP = 1e-3            # share of ambiguous ReLU signs a case may excuse (bn_ref64.AMB_CAP)
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_worker.py")
TABLES = list(T.TABLES)


def run_worker(table: str, mode: str, out: str, timeout: float) -> subprocess.CompletedProcess:
    """one child with exactly the table's knobs in its environment"""
    env = {k: v for k, v in os.environ.items() if k not in _lib.TUNING_ENV}
    env.update(T.env_of(table))
    return subprocess.run([sys.executable, WORKER, table, mode, out], env=env, timeout=timeout, capture_output=True, text=True)


def read_lines(path: str):
    return [json.loads(ln) for ln in open(path)]


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    out = {}
    for table in TABLES:
        path = str(tmp_path_factory.mktemp("tuned") / f"{table}.jsonl")
        p = run_worker(table, "routes", path, 300)
        assert p.returncode == 0, (table, p.stdout[-2000:], p.stderr[-2000:])
        lines = read_lines(path)
        assert lines[-1].get("done") and lines[-1]["table"] == table
        out[table] = {ln["case"]: ln for ln in lines[:-1]}
    return out


@pytest.mark.parametrize("table", TABLES)
def test_every_case_reports_what_the_table_declares(reports, table):
    rep, bad = reports[table], []
    cases = T.conv_cases(table) + list(S.CASES)
    assert sorted(rep) == sorted(c.name for c in cases)
    for c in cases:
        bad += [(c.name,) + b for b in T.check_line(table, c, rep[c.name])]
    assert not bad, bad[:10]
    # a pin that restates the default declaration would hide that a case stopped moving
    for name, r in T.MOVED_CONV[table].items():
        assert r != E.BY_NAME[name].route, name
    for name, (r, u, g) in T.MOVED_STEM[table].items():
        c = S.BY_NAME[name]
        assert (r, u, g) != (c.route, c.units if c.units is not None else u, c.grid if c.grid is not None else g), name


def test_the_capped_partial_rows_are_capped(reports):
    """the new BatchNorm cases exist for the cap: 37 rows with one channel chunk, 18 with two, where 1024 would give more"""
    for c in T.NEW["alt"]:
        if c.method in ("bn_stats", "bn_bwd_reduce"):
            (b,) = reports["alt"][c.name]["bound"]
            want = T.BN_PARTS // (-(-b["cgs"] // 256))
            assert b["nparts"] == want < T.nparts_rule(b["cgs"], b["pixels"], b["max_parts"], 1024), (c.name, b)


def tuned_header_routes():
    text = open(E._HDR).read()

    def block(macro):
        body = text[text.index(f"#define {macro}(X)"):].split("\n")
        lines = []
        for ln in body[1:]:
            lines.append(ln)
            if not ln.rstrip().endswith("\\"):
                break
        return re.findall(r"X\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", "\n".join(lines))
    ig = {E.IR(k, *map(int, r[:6])) | (T.COGROUPS4 if int(r[6]) else 0) for k, *r in block("SFK_IGEMM_ROUTES_TUNED")}
    wg = {E.WR(k, *map(int, r[:6])) | (T.RING5 if int(r[6]) else 0) for k, *r in block("SFK_WGRAD_ROUTES_TUNED")}
    return ig, wg


def test_the_tables_reach_exactly_the_tuned_lists_of_the_header(reports):
    ig0, wg0 = E.header_routes()
    ig, wg = tuned_header_routes()
    assert ig and wg and not ig & set(ig0) and not wg & set(wg0)
    seen_i = {ln["route"] for rep in reports.values() for ln in rep.values() if ln["kind"] == "conv_igemm"}
    seen_w = {ln["route"] for rep in reports.values() for ln in rep.values() if ln["kind"] == "conv_wgrad"}
    assert seen_i - set(ig0) == ig, ([hex(r) for r in seen_i - set(ig0) - ig], [hex(r) for r in ig - seen_i])
    assert seen_w - set(wg0) == wg, ([hex(r) for r in seen_w - set(wg0) - wg], [hex(r) for r in wg - seen_w])
    sr = S.header_routes()
    assert {ln["route"] for rep in reports.values() for ln in rep.values() if ln.get("route") is not None
            and ln["kind"].startswith("stem")} <= set(sr)


def test_ring_depth_and_pointwise_variant_have_routes_of_their_own(reports):
    alt = reports["alt"]
    for name in ("wg_bf16_dma128_ws", "wg_bf16_dma256_big"):
        assert alt[name]["route"] == E.BY_NAME[name].route | T.RING5 != E.BY_NAME[name].route
    for name in ("wg_bf16_dma256_dg_slice", "wg_bf16_dma256_dg_many", "wg_bf16_dma256_cols64"):       # these keep 3 slots
        assert alt[name]["route"] == E.BY_NAME[name].route and not alt[name]["route"] & T.RING5
    for name in ("bf16_pw_fused_one_pixel", "bf16_pw_fused_40_256"):
        assert alt[name]["route"] == E.BY_NAME[name].route | T.COGROUPS4 != E.BY_NAME[name].route
    assert not any(ln.get("route", 0) and ln["route"] & (T.RING5 | T.COGROUPS4) for t in ("narrow", "off") for ln in reports[t].values()
                   if ln["kind"] in ("conv_igemm", "conv_wgrad"))


def test_the_new_ring_cases_meet_the_runs_they_are_named_for(reports):
    for name, (tiles, target, runs) in T.RING_RUNS.items():
        ln = reports["alt"][name]
        assert T.ring_runs(ln["m"], tiles, target) == runs and ln["splits"] == len(runs), (name, ln)
    assert {r[-1] for _, _, r in T.RING_RUNS.values()} >= {1, 2, 3, 4, 5, 6}        # every run up to the ring + 1


def test_pool_cases_state_their_trips():
    per = 256 * T.POOL_BLOCKS
    items = []
    for case, fwd, bwd in T.POOL_CASES:
        it = T.pool_items(case)
        assert (fwd, bwd) == (-(-it["fwd"] // per), -(-it["bwd"] // per)), (T.pool_name(case), it)
        items += [it["fwd"], it["bwd"]]
    assert per in items and per + 1 in items and any(i > 3 * per and i % per for i in items)
    assert {(c["dtype"], (c["k"], c["s"], c["p"]) == (3, 2, 1)) for c, _, _ in T.POOL_CASES} == {(d, w) for d in (B.BF16, B.F32) for w in (True, False)}


def test_head_pool_cases_state_their_trips():
    per, items = 256 * T.POOL_BLOCKS, []
    for case, bwd, mask in T.HEAD_POOL_CASES:
        it = T.head_items(case)
        (p,) = case["parts"]
        assert tuple(p["k"]) != tuple(p["dims"]), "the window equals the map: head_pool1_*, whose grid is not capped"
        assert (bwd, mask) == (-(-it["bwd"] // per), -(-it["mask"] // per)), (case["name"], it)
        items.append((it["bwd"], it["mask"]))
    for col in (0, 1):
        seen = [i[col] for i in items]
        assert per in seen and per + 1 in seen and any(i > per and i % per for i in seen), seen
    assert any(i[0] > 3 * per and i[0] % per for i in items)


# ----------------------------------------------------------------------------- the reference alone
def _bound(case, be):
    rec = la.Recorder(be)
    case.bind(rec, "cpu")
    (sig,) = rec.calls
    return sig


NEW_FAST = [(t, c) for t in TABLES for c in T.NEW[t] if not c.slow]


@pytest.mark.parametrize("table,case", NEW_FAST, ids=[f"{t}-{c.name}" for t, c in NEW_FAST])
def test_the_reference_alone_is_inside_every_bound(table, case):
    r = la.replay(_bound(case, E.EdgeEmu()), E.EdgeEmu(), "cpu", seed=case.seed)
    assert r.ambiguous < AMB_CAP, r.ambiguous           # a condition on the inputs: a case that misses it gets another seed
    assert r.ok, (r.verdicts, r.untouched_bad)


def test_the_slow_new_cases_are_the_p8_ones():
    assert [c.name for t in TABLES for c in T.NEW[t] if c.slow] == [c.name for c in T.NEW["alt"] if c.name.startswith("p8_")]


@pytest.mark.parametrize("case", [c for c, _, _ in T.POOL_CASES], ids=T.pool_name)
def test_the_pool_reference_alone(case):
    vs = B.check_pool(EmuBackend(), "cpu", case)
    assert not B.failures(vs), B.failures(vs)[:4]


@pytest.mark.parametrize("case", [c for c, _, _ in T.HEAD_POOL_CASES], ids=lambda c: c["name"])
def test_the_head_pool_reference_alone(case):
    vs = H.check_pool(EmuBackend(), "cpu", case)
    assert not H.failures(vs), H.failures(vs)[:4]


# ----------------------------------------------------------------------------- mutations
def _zero_rows(lo, hi):
    return lambda p, _: _rows(p.y)[lo:hi].zero_()


def _keep_rows(lo):
    return dict(snap=lambda p: _rows(p.y)[lo:].clone(), post=lambda p, s: _rows(p.y)[lo:].copy_(s))


def _flip_mask_byte(p):
    bits = p.relu_out_bits.clone()
    bits[(p.y.pixels - 1) * (p.cout // 8)] ^= 0xFF            # the first channel group of the last pixel
    return dataclasses.replace(p, relu_out_bits=bits)


def _second_chunk_lost(p, _):
    X, D = _rows(p.x).float(), _rows(p.dy).float()
    p.dw[: p.cout * p.wtaps * p.cin].view(p.cout, p.wtaps, p.cin)[:, 0, :] -= D[32:].t() @ X[32:]


# (the P8 mutations run on the 16,385-pixel case that the table moves to the 224-row tile: 73 whole tiles and one of 33 rows)
CONV_MUTATIONS = {
    "rows 224 .. 255 of a P8 tile written": ("alt", "bf16_p8_256", "conv_igemm", dict(post=_zero_rows(224, 256))),
    "partial rows of the last 224-row tile dropped": ("alt", "bf16_p8_256", "conv_igemm", _keep_rows(73 * 224)),
    "channels 4 .. 7 of an 8-channel group dropped in a fused epilogue": ("narrow", "bf16_reg64_ep_res_relu", "conv_igemm", dict(
        snap=lambda p: _rows(p.y)[:, 4:8].clone(), post=lambda p, s: _rows(p.y)[:, 4:8].copy_(s))),
    "ReLU-mask byte of a BatchNorm-backward pass wrong": ("narrow", "bf16_reg64_bnb5", "conv_igemm", dict(pre=_flip_mask_byte)),
    "a ring run of two chunks counted as one": ("alt", "wg_ring5_128_run2", "conv_wgrad", dict(post=_second_chunk_lost)),
}


@pytest.mark.parametrize("what", list(CONV_MUTATIONS), ids=lambda s: s.replace(" ", "_"))
def test_replay_refuses_the_mutation(what):
    table, name, method, how = CONV_MUTATIONS[what]
    case = T.NEW_BY_NAME[table].get(name) or E.BY_NAME[name]
    assert case.method == method
    sig = _bound(case, E.EdgeEmu())
    assert la.replay(sig, E.EdgeEmu(), "cpu", seed=case.seed).ok
    r = la.replay(sig, conv_mutant(method, **how), "cpu", seed=case.seed)
    assert not r.ok, (what, r.verdicts)


def test_replay_refuses_a_dropped_trailing_half_pair_of_a_v2_case():
    """35 frames: 17 pairs and a half pair in three chunks on the whole-tile kernel (SFK_STEM3 = 0)"""
    name = "v4_k5_c8_t35_7x4"
    assert T.MOVED_STEM["alt"][name][0] == S.SR("V2", 1, 1, 5)
    case = S.BY_NAME[name]
    _, _, sig = S.bound(case, EmuBackend())
    assert la.replay(sig, EmuBackend(), "cpu", seed=case.seed).ok
    m = stem_mutant(case.method, snap=lambda a: a["y"].view5()[:, -1].clone(), post=lambda a, s: a["y"].view5()[:, -1].copy_(s))
    assert not la.replay(sig, m, "cpu", seed=case.seed).ok


def test_check_pool_refuses_a_dropped_second_trip():
    """513 items on 512 threads: the one element group of the second trip keeps its old bytes"""
    case = next(c for c, fwd, _ in T.POOL_CASES if T.pool_items(c)["fwd"] == 256 * T.POOL_BLOCKS + 1)

    class M(EmuBackend):
        def maxpool_fwd(self, x, y, argmax, k, s, p):
            run = super().maxpool_fwd(x, y, argmax, k, s, p)

            def r(stream):
                last = y.view5()[-1, -1, -1, -1]
                keep = last.clone()
                run(stream)
                last.copy_(keep)
            return r
    assert not B.failures(B.check_pool(EmuBackend(), "cpu", case))
    assert B.failures(B.check_pool(M(), "cpu", case))
