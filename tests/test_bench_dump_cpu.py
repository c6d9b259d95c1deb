"""bench.py --dump-outputs on CPU (the engine over tests/emu_backend.py): what it writes after a training step is float32,
bounded in size, the same from run to run, and is what the step computed (loss, logits, state, gradients)."""
import os
import sys

import numpy as np
import torch

from test_engine_cpu import make_inputs, make_models
from video_classification_amd.train import TrainStep

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _run_and_dump(out_dir, sample=None, steps=2, restore_before_last=False):
    _, m = make_models(ref_style=True)
    eng = m.engine
    start = bench.StepState(eng)
    x = make_inputs(ref_style=True)
    labels = torch.tensor([1, 4])
    step = TrainStep(eng, lr=1e-2, use_graph=False)
    for i in range(steps):
        if restore_before_last and i == steps - 1:
            start.restore()
        loss = step(x[0], x[1], labels)
    old = bench.DUMP_SAMPLE
    if sample is not None:
        bench.DUMP_SAMPLE = sample
    try:
        bench.dump_outputs(str(out_dir), eng, eng._plan_for(x[0], x[1], None, True), loss)
    finally:
        bench.DUMP_SAMPLE = old
    return eng, float(loss[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_is_float32_bounded_and_repeats(tmp_path):
    _, loss, a = _run_and_dump(tmp_path / "a")
    assert set(a) == {"loss", "logits", "state_sample", "grad_sample"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].shape == (1,) and a["loss"][0] == np.float32(loss)
    assert a["logits"].shape == (2, 7)
    assert a["state_sample"].shape == a["grad_sample"].shape == (bench.DUMP_SAMPLE,)
    # same inputs, same outputs
    _, _, b = _run_and_dump(tmp_path / "b")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_dump_outputs_is_the_state_and_the_gradients(tmp_path):
    # a sample larger than the model: the whole state / gradient, flattened in sorted key order
    eng, _, a = _run_and_dump(tmp_path / "a", sample=1 << 30)
    sd = eng.state_dict()                                          # (taken after the dump: the gradient read-out restored P)
    np.testing.assert_array_equal(a["state_sample"], np.concatenate([sd[k].reshape(-1).float().numpy() for k in sorted(sd)]))
    keep = eng.P.data.clone()
    eng.P.data.copy_(eng.G)
    gsd = eng.state_dict()
    eng.P.data.copy_(keep)
    gk = sorted(k for k in gsd if k not in eng.dead and not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    np.testing.assert_array_equal(a["grad_sample"], np.concatenate([gsd[k].reshape(-1).float().numpy() for k in gk]))
    assert np.abs(a["grad_sample"]).max() > 0


def test_dump_outputs_samples_large_outputs_at_fixed_positions(tmp_path):
    _, _, a = _run_and_dump(tmp_path / "a", sample=1000)
    _, _, b = _run_and_dump(tmp_path / "b", sample=1000)
    assert a["state_sample"].shape == (1000,) and a["grad_sample"].shape == (1000,)
    np.testing.assert_array_equal(a["state_sample"], b["state_sample"])
    np.testing.assert_array_equal(a["grad_sample"], b["grad_sample"])


def test_step_state_restore_repeats_the_first_step(tmp_path):
    """bench.py --dump-outputs restores StepState before its last timed step: from there a trained engine computes exactly
    what a fresh one computes in its first step (weights, Adam, BatchNorm running statistics, dropout seed)."""
    _, _, first = _run_and_dump(tmp_path / "fresh", sample=1 << 30, steps=1)
    _, _, last = _run_and_dump(tmp_path / "restored", sample=1 << 30, steps=3, restore_before_last=True)
    _, _, trained = _run_and_dump(tmp_path / "trained", sample=1 << 30, steps=3)
    for k in first:
        np.testing.assert_array_equal(first[k], last[k])
    assert not np.array_equal(first["state_sample"], trained["state_sample"])   # (without the restore the step differs)
