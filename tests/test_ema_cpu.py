"""The weight EMA on the CPU (include/sfk_ema.h, ema.WeightEma, TrainStep's ema_decay / ema_warmup, MODEL.EMA_*,
tests/ref_ema.py, tests/emu_ema.py): the reference against float64 torch.lerp and timm's warm-up, the ctypes binding of the
new header and its host-side rejections, mutants of the emulated backend against the checks the GPU file runs, and the
wiring through TrainStep and both trainers."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import head_ref64 as H
import ref_ema as R
from emu_ema import EmuEmaBackend
from video_classification_amd import gesture_v2 as v2
from video_classification_amd import train as v1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "CropLHand"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the reference
def test_ref_ema_is_the_plain_expression_and_stays_within_its_bound_of_float64_lerp():
    worst = 0.0
    for seed, n in enumerate([4099, 2048, 257, 64, 8, 1]):
        p, e = R.ema_values(n, seed)
        assert float(p.abs().min()) >= 2.0 ** -20 and float(p.abs().max()) <= 2.0 ** 20 and bool((p[3::7] == e[3::7]).all())
        for decay in R.DECAYS:
            for warmup in (False, True):
                for t in R.STEPS:
                    w = R.ema_weight(decay, warmup, t)
                    got = R.ref_ema(e, p, w)
                    wt = torch.tensor(w, dtype=torch.float32)
                    assert torch.equal(got, e + wt * (p - e))
                    # every op rounded on its own, restated in float64
                    d = (p.double() - e.double()).float()
                    m = (wt.double() * d.double()).float()
                    assert torch.equal(got, (e.double() + m.double()).float())
                    assert torch.equal(got[3::7], e[3::7])                   # p == e: the average stays, exactly
                    err = (got.double() - R.ref_lerp64(e, p, w)).abs()
                    bound = R.ema_bound(e, p, w)
                    assert bool((err <= bound).all()), (n, decay, warmup, t, float((err / bound.clamp_min(1e-300)).max()))
                    worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                    # no intermediate is subnormal
                    tiny = 2.0 ** -126
                    assert all(bool(((x == 0) | (x.abs() >= tiny)).all()) for x in (d, m, got))
    print(f"worst error / bound {worst:.3f}")
    assert 0.05 < worst <= 1.0


def test_rate_follows_timms_warmup():
    for decay in (0.9, 0.9999):
        for t in list(range(1, 13)) + [10 ** 6]:
            want = min(decay, (1 + t) / (10 + t))
            assert R.ema_rate(decay, True, t) == want and R.ema_rate(decay, False, t) == decay
            assert R.ema_weight(decay, True, t) == H.f32(1.0 - want)
    assert R.ema_rate(0.9, True, 1) == 2 / 11 and R.ema_rate(0.9999, True, 10 ** 6) == 0.9999
    assert R.ema_weight(0.0, False, 5) == 1.0


# ------------------------------------------------------------------ the binding of include/sfk_ema.h
def test_ema_table_matches_its_header(lib, tmp_path):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_ema.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_EMA) == ["sfk_ema_abi_version", "sfk_ema_swap", "sfk_ema_update"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG, _lib.SIGNATURES_OPTIM, _lib.SIGNATURES_GROUPS,
                  _lib.SIGNATURES_MIX):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_EMA[n]), n
    assert lib.sfk_ema_abi_version() == _lib.EMA_ABI_VERSION == 1 == int(re.search(r"#define\s+SFK_EMA_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.EMA_MAX_TENSORS == 4096 == int(re.search(r"#define\s+SFK_EMA_MAX_TENSORS\s+(\d+)", src).group(1))
    sizes = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "float": 4, "double": 8}
    for cname, ctype, size in (("sfk_ema_tensor", _lib._EmaTensor, 24), ("sfk_ema_desc", _lib._EmaDesc, 64)):
        body = re.search(r"typedef struct \{([^{}]*)\} " + cname + ";", src).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
            for nm in m.group(3).replace("*", "").split(","):
                fields.append((nm.strip(), 8 if m.group(2) else sizes[m.group(1)]))
        assert [(f, ctypes.sizeof(t)) for f, t in ctype._fields_] == fields
        assert ctypes.sizeof(ctype) == size
    assert _lib.new_ema_desc().struct_size == 64
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_ema.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                    'sizeof(sfk_ema_desc), offsetof(sfk_ema_desc, table), offsetof(sfk_ema_desc, decay), offsetof(sfk_ema_desc, step), '
                    'sizeof(sfk_ema_tensor), offsetof(sfk_ema_tensor, n)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    D, T = _lib._EmaDesc, _lib._EmaTensor
    assert [int(v) for v in out] == [ctypes.sizeof(D), D.table.offset, D.decay.offset, D.step.offset, ctypes.sizeof(T), T.n.offset]


def _good_ema(p, e, table, step):
    from video_classification_amd import _lib
    d = _lib.new_ema_desc()
    d.p, d.e, d.count, d.table, d.ntensors = p.data_ptr(), e.data_ptr(), p.numel(), ctypes.addressof(table), 2
    d.decay, d.warmup, d.step = 0.9, 1, step.data_ptr()
    return d


def test_ema_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    from video_classification_amd import _lib
    p, e, step = torch.ones(64), torch.zeros(64), torch.zeros(1, dtype=torch.int64)
    a, b = torch.ones(8), torch.zeros(8)
    table = (_lib._EmaTensor * 2)(_lib._EmaTensor(a.data_ptr(), b.data_ptr(), 8, 0), _lib._EmaTensor(a.data_ptr(), b.data_ptr(), 8, 0))
    B = ctypes.byref
    both = [("struct_size", 8), ("struct_size", 56), ("struct_size", 72), ("p", None), ("e", None), ("count", 0), ("count", -4),
            ("ntensors", -1), ("ntensors", 4097), ("table", None)]
    only_update = [("step", None), ("decay", 1.0), ("decay", -0.01), ("decay", 1.5), ("decay", float("nan"))]
    for field, value in both + only_update:
        d = _good_ema(p, e, table, step)
        setattr(d, field, value)
        assert lib.sfk_ema_update(B(d), None) == -1, (field, value)
    for field, value in both:
        d = _good_ema(p, e, table, step)
        setattr(d, field, value)
        assert lib.sfk_ema_swap(B(d), None) == -1, (field, value)
    assert lib.sfk_ema_update(None, None) == -1 and lib.sfk_ema_swap(None, None) == -1
    d = _good_ema(p, e, table, step)
    d.count = (1 << 42) + 1
    assert lib.sfk_ema_update(B(d), None) == -2 and lib.sfk_ema_swap(B(d), None) == -2
    assert float(p.min()) == 1 and float(e.abs().max()) == 0 and int(step[0]) == 0 and float(b.abs().max()) == 0


# ------------------------------------------------------------------ the emulated backend and its mutants
def _update_verdicts(be):
    vs = []
    for case in R.update_cases():
        vs += R.check_ema_update(be, "cpu", *case)
    return vs


def _swap_verdicts(be):
    vs = []
    for case in R.swap_cases():
        vs += R.check_ema_swap(be, "cpu", *case)
    return vs


def test_cases_cover_what_the_header_distinguishes():
    cases = R.update_cases()
    assert {c[0] for c in cases} == set(R.COUNTS) and {c[1] for c in cases} == set(R.TABLES)
    assert {c[2] for c in cases} == set(R.OFFSETS) and {c[3] for c in cases} == set(R.DECAYS)
    assert {(c[3], c[4], c[5]) for c in cases} >= {(d, w, t) for d in R.DECAYS for w in (False, True) for t in R.STEPS}
    assert {(c[0], c[1]) for c in R.swap_cases()} >= {(c, t) for c in R.COUNTS for t in R.TABLES}


def test_emulated_backend_passes_the_checks_the_gpu_file_runs():
    be = EmuEmaBackend()
    vs = _update_verdicts(be) + _swap_verdicts(be)
    assert len(vs) > 500 and not H.failures(vs), H.failures(vs)[:5]
    assert set(be.launches) == {"ema_update", "ema_swap"}


def _mutant(**flags):
    return type("Mutant", (EmuEmaBackend,), flags)()


@pytest.mark.parametrize("flags,run,word", [
    (dict(warmup_ignored=True), _update_verdicts, "bits"), (dict(step_before_increment=True), _update_verdicts, "bits"),
    (dict(table_skipped=True), _update_verdicts, "table"), (dict(last_element_skipped=True), _update_verdicts, "arena bits"),
    (dict(swap_copies=True), _swap_verdicts, "exchanged"), (dict(convex_form=True), _update_verdicts, "bits")],
    ids=["warmup_ignored", "t_minus_1", "table_skipped", "last_element_skipped", "swap_copies", "convex_form"])
def test_mutants_are_refused(flags, run, word):
    bad = H.failures(run(_mutant(**flags)))
    assert bad and all(word in v.name or "twice" in v.name for v in bad), bad[:5]


# ------------------------------------------------------------------ TrainStep
def _mini(backend=None, seed=0):
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=torch.float32, device="cpu", backend=backend or EmuEmaBackend(), seed=seed)


def _batches(k, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 7, 4, 64, 64, generator=g), torch.randint(0, 7, (2,), generator=g)) for _ in range(k)]


def test_ema_decay_zero_builds_nothing():
    be = EmuEmaBackend()
    m = _mini(be)
    st = v1.TrainStep(m.engine, lr=1e-3, ema_decay=0.0, ema_warmup=True)
    assert st.ema is None
    m.train()
    for x, y in _batches(2):
        st(x[:, :5], x[:, 5:], y)
    ops = next(iter(st._cache.values()))["ops"]
    assert sorted(ops) == ["adam", "loss", "zero_grad", "zero_loss"]
    assert not [n for n in be.launches if n.startswith("ema")] and m.engine.ema_P is None and m.engine.ema_table is None


def test_train_step_keeps_the_reference_recursion():
    be = EmuEmaBackend()
    m = _mini(be)
    eng = m.engine
    st = v1.TrainStep(eng, lr=1e-2, ema_decay=0.9, ema_warmup=True)
    assert st.ema is not None and torch.equal(eng.ema_P, eng.P.data) and eng.ema_P.data_ptr() != eng.P.data.data_ptr()
    assert len(eng.ema_stat_pairs()) == 2 * len(eng.layers) == eng.ema_table.ntensors
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in eng.ema_stat_pairs())
    m.train()
    batches = iter(_batches(4))

    def one():
        x, y = next(batches)
        st(x[:, :5], x[:, 5:], y)
    be.launches.clear()
    vs = R.check_route(eng, one, 4, 0.9, True)
    assert not H.failures(vs), H.failures(vs)[:5]
    assert [n for n in be.launches if n.startswith("ema")] == ["ema_update"] * 4
    assert be.launches[-1] == "ema_update"                                        # after the optimizer launch
    ops = next(iter(st._cache.values()))["ops"]
    assert sorted(ops) == ["adam", "ema", "loss", "zero_grad", "zero_loss"]
    # one state per engine: a second TrainStep shares it
    st2 = v1.TrainStep(eng, lr=1e-2, ema_decay=0.5)
    assert st2.ema.eng.ema_P is eng.ema_P and int(eng.ema_step[0]) == 4


def test_ema_decay_outside_its_range_is_refused():
    m = _mini()
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            v1.TrainStep(m.engine, lr=1e-3, ema_decay=bad)


def test_applied_reset_and_state_dicts():
    from video_classification_amd.ema import WeightEma
    m = _mini()
    eng = m.engine
    ema = WeightEma(eng, 0.9)
    eng.ema_P.mul_(0.5)
    for _, avg in eng.ema_stat_pairs():
        avg.add_(0.25)
    live, avg = R.live_snapshot(eng), R.ema_snapshot(eng)
    nbt = eng.layers[0].nbt.clone().fill_(7)
    eng.layers[0].nbt.fill_(7)
    with ema.applied():
        assert all(torch.equal(a, b) for a, b in zip(R.live_snapshot(eng), avg))
        inside = eng.state_dict()
    assert all(torch.equal(a, b) for a, b in zip(R.live_snapshot(eng), live))
    assert all(torch.equal(a, b) for a, b in zip(R.ema_snapshot(eng), avg))
    sd, live_sd = ema.state_dict(), eng.state_dict()
    assert sorted(sd) == sorted(live_sd) and all(torch.equal(sd[k], inside[k]) for k in sd)
    L = eng.layers[0]
    assert torch.equal(sd[L.cb.norm_key + ".running_var"], live_sd[L.cb.norm_key + ".running_var"] + 0.25)
    assert torch.equal(sd[L.cb.conv_key + ".weight"], live_sd[L.cb.conv_key + ".weight"] * 0.5)
    assert int(sd[L.cb.norm_key + ".num_batches_tracked"]) == 7 == int(nbt[0])
    # load_state_dict fills the average and leaves the live model alone
    other = {k: (v + 1 if v.is_floating_point() else v * 0) for k, v in live_sd.items()}
    ema.load_state_dict(other)
    assert all(torch.equal(a, b) for a, b in zip(R.live_snapshot(eng), live)) and int(eng.layers[0].nbt[0]) == 7
    back = ema.state_dict()
    assert all(torch.equal(back[k], other[k]) for k in other if other[k].is_floating_point() and k not in eng.dead)
    assert all(torch.equal(back[k], live_sd[k]) for k in eng.dead)               # the dead tensors stay the live model's
    eng.ema_step.fill_(5)
    ema.reset()
    assert all(torch.equal(a, b) for a, b in zip(R.ema_snapshot(eng), live)) and int(eng.ema_step[0]) == 0


# ------------------------------------------------------------------ config and trainers
def _cfg(name="slowfast-LHand", bs=2, **model):
    from video_classification_amd.config import get_cfg
    cfg = get_cfg()
    cfg.CHALEARN.ROOT = "/nonexistent"
    cfg.CHALEARN.BATCH_SIZE = bs
    cfg.CHALEARN.CLIP_LEN = 4
    cfg.CHALEARN.NUM_CLASS = 7
    cfg.MODEL.NAME = name
    cfg.MODEL.R3D_INPUT = KEY
    cfg.MODEL.INPUT_SIZE = 64
    cfg.MODEL.DEPTH = 18
    cfg.MODEL.RES2D_BACKEND = "engine"
    cfg.MODEL.LR = 1e-2
    cfg.MODEL.MAX_EPOCH = 2
    cfg.NUM_CPU = 0
    for k, v in model.items():
        setattr(cfg.MODEL, k, v)
    return cfg


def test_config_defaults():
    from video_classification_amd.config import get_cfg
    m = get_cfg().MODEL
    assert (m.EMA_DECAY, m.EMA_WARMUP, m.EMA_EVAL) == (0.0, False, "ema")
    assert v1.ema_settings(get_cfg()) == (0.0, False, "ema")
    assert v1.ema_settings(_cfg(EMA_DECAY=0.99, EMA_WARMUP=True, EMA_EVAL="both")) == (0.99, True, "both")
    for bad in (dict(EMA_DECAY=1.0), dict(EMA_DECAY=-0.5), dict(EMA_EVAL="average")):
        with pytest.raises(ValueError, match="EMA_"):
            v1.ema_settings(_cfg(**bad))


def make_trainer(which, tmp_path, device="cpu", backend=None, **model):
    """a trainer of two mini epochs of two steps that writes real checkpoints under tmp_path"""
    cfg = _cfg("gesture-v2" if which == "v2" else "slowfast-LHand", **model)
    cfg.CHALEARN.ROOT = str(tmp_path)
    cfg.DEBUG = False
    if which == "v2":
        tr = v2.SyntheticGesture(cfg, "train", num_videos=4, seed=1, h=48, w=64, min_box=8)
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
        return v2.Trainer(cfg, train_set=tr, test_set=te, device=device, backend=backend)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    return v1.Trainer(cfg, train_set=tr, test_set=te, device=device, backend=backend)


def check_trainer_epochs(t, capsys, which_eval):
    """train() of two epochs of two steps.  Around every averaged region of train() (the epoch's evaluation with its
    checkpoint, and the final save) the live arena and statistics are snapshotted before the region is entered and after it
    is left: they must hold the same bits, and so must the average.  run_eval inside the region sees the averaged arena and
    statistics (with 'live', the live ones); with 'both' the evaluation before it sees the live ones.  Every saved .ckpt
    equals ema.state_dict() (with 'live', the live state_dict) as it stood when its region was entered.  The second epoch
    trains on after a swap-back."""
    import contextlib
    eng = t.model.engine
    ema = t.step.ema
    averaged_mode = which_eval != "live"
    assert ema is not None and torch.equal(eng.ema_P, eng.P.data) and int(eng.ema_step[0]) == 0
    marks, seen, inside = [], [], [False]
    run_eval, averaged = t.run_eval, t._averaged

    def eval_spy(*a, **kw):
        seen.append((inside[0], len(marks), eng.P.data.detach().cpu().clone(), eng.layers[0].rv.detach().cpu().clone()))
        return run_eval(*a, **kw)

    @contextlib.contextmanager
    def region():
        mark = dict(live=R.live_snapshot(eng), avg=R.ema_snapshot(eng), step=int(eng.ema_step[0]),
                    want={k: v.cpu() for k, v in (ema.state_dict() if averaged_mode else eng.state_dict()).items()})
        marks.append(mark)
        inside[0] = True
        with averaged():
            yield
        inside[0] = False
        mark["live_after"], mark["avg_after"] = R.live_snapshot(eng), R.ema_snapshot(eng)
    t.run_eval, t._averaged = eval_spy, region
    t.max_historical_acc = -1.0                                                   # epoch 0's checkpoint is written whatever the accuracy
    t.train()
    out = capsys.readouterr().out
    assert len(marks) == 3 and [m["step"] for m in marks] == [2, 4, 4] and int(eng.ema_step[0]) == 4
    for m in marks:
        assert not torch.equal(m["live"][0], m["avg"][0])
        assert all(torch.equal(R._bits(a), R._bits(b)) for a, b in zip(m["live"], m["live_after"]))
        assert all(torch.equal(R._bits(a), R._bits(b)) for a, b in zip(m["avg"], m["avg_after"]))
    assert not torch.equal(marks[0]["live"][0], marks[1]["live"][0])              # epoch 1 trained on after the swap-back
    assert not torch.equal(marks[0]["avg"][0], marks[1]["avg"][0])
    assert len(seen) == (4 if which_eval == "both" else 2)
    for was_inside, nmarks, P, rv in seen:
        if was_inside:
            side = marks[nmarks - 1]["avg" if averaged_mode else "live"]
        else:                                                                     # 'both': the live evaluation before the region
            assert which_eval == "both"
            side = marks[nmarks]["live"]
        assert torch.equal(R._bits(P), R._bits(side[0])) and torch.equal(R._bits(rv), R._bits(side[2]))   # [2]: layer 0's variance
    assert sum(1 for s_ in seen if s_[0]) == 2
    assert ("Live Accuracy" in out) == (which_eval == "both") and ("EMA Accuracy" in out) == averaged_mode
    ckpts = {int(str(path).rsplit("_e", 1)[1].split(".")[0]): path for path in t.ckpt_dir.glob("*.ckpt")}
    assert set(ckpts) == {0, 1}
    for epoch, path in ckpts.items():
        sd, want = torch.load(path, map_location="cpu", weights_only=True), marks[0 if epoch == 0 else 2]["want"]
        assert sorted(sd) == sorted(want) and all(torch.equal(sd[k], want[k]) for k in sd), path
    final = ema.state_dict() if averaged_mode else eng.state_dict()
    assert all(torch.equal(marks[2]["want"][k], final[k].cpu()) for k in final)
    return out


@pytest.mark.parametrize("which,which_eval", [("v1", "ema"), ("v1", "both"), ("v1", "live"), ("v2", "ema"), ("v2", "both")])
def test_trainer_epochs_evaluate_and_save_the_average(which, which_eval, tmp_path, capsys):
    be = EmuEmaBackend()
    t = make_trainer(which, tmp_path, backend=be, EMA_DECAY=0.9, EMA_WARMUP=True, EMA_EVAL=which_eval)
    be.launches.clear()
    check_trainer_epochs(t, capsys, which_eval)
    ema = [n for n in be.launches if n.startswith("ema")]
    # two swaps each: applied() in train()'s three regions, the check's ema.state_dict() before each, and its last one
    assert ema.count("ema_update") == 4 and ema.count("ema_swap") == (0 if which_eval == "live" else 14)


def test_trainers_with_the_default_build_nothing(tmp_path):
    be = EmuEmaBackend()
    t = make_trainer("v1", tmp_path, backend=be)
    assert t.step.ema is None and t._ema_kwargs() == {} and t.model.engine.ema_P is None
    t.train_epoch()
    assert not [n for n in be.launches if n.startswith("ema")]


def test_res2d_with_the_torch_backend_refuses_ema(tmp_path):
    cfg = _cfg("res2d", RES2D_BACKEND="torch", EMA_DECAY=0.9)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    with pytest.raises(ValueError, match="EMA_DECAY.*res2d.*torch"):
        v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuEmaBackend())
    cfg = _cfg("res2d", EMA_DECAY=0.9)                           # the engine backend carries it
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=EmuEmaBackend())
    assert t.step.ema is not None
