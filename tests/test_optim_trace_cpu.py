"""Every optimizer-side backend call TrainStep makes -- which method, over which slice of which arena, with which scalars --
pinned to tests/golden/optim_launch_trace.json, which was recorded with this same recorder (tests/optim_trace.py) before the
three optimizer routes were folded into optim.Optimizer: the depth-18 mini model on the emulated backend, two clips, two
steps, Adam and SGD under every setting that picks another launch, without a reducer and (Adam) with a world-1 GradReducer,
and the split pair built directly (TrainStep asks for it on a CUDA device only).  Each case also pins which optimizer state
the engine holds afterwards, and that constructing the TrainStep allocated none of it."""
import json
import os

import pytest
import torch

from emu_optim import EmuOptimBackend
from optim_trace import STATE, LaunchTrace, state_present
from test_optim_cpu import _batches, _mini

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "optim_launch_trace.json")
TABLE = [1e-4, 3e-4, 2e-4]
SETTINGS = {
    "defaults": {},
    "table": dict(lr_table=TABLE),
    "l2-weights": dict(weight_decay=0.1, decay_mode="l2", decay_scope="weights"),
    "l2-all": dict(weight_decay=0.1, decay_mode="l2", decay_scope="all"),
    "decoupled": dict(weight_decay=0.1, decay_mode="decoupled"),
    "clip": dict(clip_grad_norm=0.5),
    "table-decay-clip": dict(lr_table=TABLE, weight_decay=0.1, decay_mode="l2", clip_grad_norm=0.5),
}
SGD_KW = dict(momentum=0.9, dampening=0.1, nesterov=False)


def _step_cases():
    for opt in ("adam", "sgd"):
        for name in SETTINGS:
            if not (opt == "sgd" and name == "decoupled"):
                yield f"{opt}-{name}"
    for name in SETTINGS:
        yield f"adam-{name}-reducer"


def _split_cases():
    return [f"split-{name}" for name, kw in SETTINGS.items() if "clip_grad_norm" not in kw]


def _split_pair(eng, cut, kw):
    """(main, tail, set_tail): the split builder, called directly"""
    from video_classification_amd.optim import Optimizer
    return Optimizer(eng, lr=1e-3, **kw).split_ops(cut)


def record_step_case(case):
    from video_classification_amd import dist as sdist
    from video_classification_amd.train import TrainStep
    opt, rest = case.split("-", 1)
    reducer = rest.endswith("-reducer")
    kw = dict(SETTINGS[rest[:-len("-reducer")] if reducer else rest], **(SGD_KW if opt == "sgd" else {}))
    m = _mini(backend=EmuOptimBackend())
    eng = m.engine
    tr = LaunchTrace(eng)
    st = TrainStep(eng, lr=1e-3, optimizer=opt, reducer=sdist.GradReducer(eng.G, bucket_mb=0.25) if reducer else None, **kw)
    assert state_present(eng) == [], "constructing a TrainStep allocates no optimizer state"
    assert st.grad_norm is None
    m.train()
    for x, y in _batches(2):
        st(x[:, :5], x[:, 5:], y)
    ops = next(iter(st._cache.values()))["ops"]
    assert (st.grad_norm is None) == ("clip_grad_norm" not in kw) and (st.grad_norm is None or st.grad_norm is eng.grad_norm)
    return dict(tr.take(), state=state_present(eng), ops=sorted(ops))


def record_split_case(case):
    kw = SETTINGS[case[len("split-"):]]
    m = _mini(backend=EmuOptimBackend())
    eng = m.engine
    tr = LaunchTrace(eng)
    cut = eng.layers[1].w_off                                    # the first layer's filters | the rest
    assert 0 < cut < eng.fc_b_off and cut % 4 == 0
    main, tail, set_tail = _split_pair(eng, cut, kw)
    gen = torch.Generator().manual_seed(3)
    for s in (1, 2):
        eng.G.copy_(torch.randn(eng.arena_numel, generator=gen))
        main(0)
        set_tail()
        assert int(eng.adam_step[0]) == s and int(eng.adam_step_tail[0]) == s - 1
        tail(0)
        assert int(eng.adam_step[0]) == int(eng.adam_step_tail[0]) == s
    return dict(tr.take(), state=state_present(eng), cut=cut, numel=eng.arena_numel)


def record(case):
    return record_split_case(case) if case.startswith("split-") else record_step_case(case)


CASES = list(_step_cases()) + _split_cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES) and len(CASES) == 13 + 7 + 5


@pytest.mark.parametrize("case", CASES)
def test_launch_trace_equals_the_recording(golden, case):
    got, want = record(case), golden[case]
    assert got["built"] == want["built"]
    assert got["ran"] == want["ran"]
    assert got["state"] == want["state"] and set(got["state"]) <= set(STATE)
    assert {k: got[k] for k in got if k not in ("built", "ran", "state")} == {k: want[k] for k in want if k not in ("built", "ran", "state")}
