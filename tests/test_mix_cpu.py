"""Mixup, CutMix and label smoothing on the CPU (include/sfk_mix.h, input_pipeline.draw_mix / ClipMix, TrainStep's
label_smoothing and mix, tests/ref_mix.py, tests/emu_mix.py): the draws, the row validation, the float64 restatement of the
loss against torch's own soft-target cross-entropy, the ctypes binding of the new header and its host-side rejections,
mutants of the emulated backend against the checks the GPU file runs, and the wiring through both trainers."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import head_ref64 as H
import ref_mix as R
from emu_mix import EmuMixBackend
from video_classification_amd import gesture_v2 as v2
from video_classification_amd import train as v1
from video_classification_amd.input_pipeline import ClipMix, draw_mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "CropLHand"                                                               # 64 x 64 crops


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from video_classification_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the draws
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("n", [1, 2, 5, 6])
def test_draw_mix_pairs_by_the_flip_and_partners_are_mutual(n):
    rows = draw_mix(n, 32, 48, 0.8, 1.0, generator=_gen(n))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, 8)
    p = rows[:, 0].long()
    assert p.tolist() == [n - 1 - i for i in range(n)] and torch.equal(p[p], torch.arange(n))
    if n % 2:
        assert rows[n // 2].tolist() == [n // 2, 1, 0, 0, 0, 0, 1, 0]            # the middle clip: a self pair, identity
    for i in range(n // 2):
        assert torch.equal(rows[i, 1:], rows[n - 1 - i, 1:])                     # both members share the draw
    assert float(rows[:, 7].abs().max()) == 0
    ClipMix.validate(rows, 32, 48)


def test_draw_mix_prob_zero_and_alphas_zero_give_identity_rows():
    ident = R.identity_rows(6)
    for kw in (dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0), dict(mixup_alpha=0.0, cutmix_alpha=0.0)):
        rows = draw_mix(6, 32, 32, generator=_gen(1), **kw)
        assert torch.equal(rows[:, 1:], ident[:, 1:])
    assert torch.equal(draw_mix(6, 32, 32, generator=_gen(1)), ident)            # no alpha: not even a pairing


def test_draw_mix_modes_weights_and_seed():
    h, w = 24, 40
    mixup = draw_mix(400, h, w, 0.8, 0.0, generator=_gen(2))
    assert float(mixup[:, 2:6].abs().max()) == 0 and torch.equal(mixup[:, 1], mixup[:, 6])
    assert 0 <= float(mixup[:, 1].min()) < 0.1 and 0.9 < float(mixup[:, 1].max()) <= 1
    cut = draw_mix(400, h, w, 0.0, 1.0, generator=_gen(3))
    assert bool((cut[:, 1] == 1).all())
    y0, x0, y1, x1 = (cut[:, i] for i in range(2, 6))
    assert bool(((y0 >= 0) & (x0 >= 0) & (y1 <= h) & (x1 <= w) & (y0 <= y1) & (x0 <= x1)).all())
    area = ((y1 - y0) * (x1 - x0)).tolist()
    assert cut[:, 6].tolist() == [torch.tensor(1.0 - a / float(h * w), dtype=torch.float32).item() for a in area]   # exactly
    assert len(set(area)) > 50 and bool((y0 == 0).any()) and bool((x1 == w).any())          # boxes differ; some are clipped
    both = draw_mix(400, h, w, 0.8, 1.0, switch_prob=0.5, generator=_gen(4))
    is_cut = (both[:, 1] == 1) & (both[:, 6] < 1)
    assert 0.3 < float(is_cut.float().mean()) < 0.7
    half = draw_mix(400, h, w, 0.8, 0.0, prob=0.5, generator=_gen(5))
    assert 0.3 < float((half[:, 1] == 1).float().mean()) < 0.7
    assert torch.equal(draw_mix(9, h, w, 0.8, 1.0, generator=_gen(6)), draw_mix(9, h, w, 0.8, 1.0, generator=_gen(6)))
    assert not torch.equal(draw_mix(9, h, w, 0.8, 1.0, generator=_gen(6)), draw_mix(9, h, w, 0.8, 1.0, generator=_gen(7)))


# ------------------------------------------------------------------ ClipMix.load
def test_clip_mix_load_keeps_one_table_and_refuses_bad_rows():
    cm = ClipMix("cpu", EmuMixBackend(), batch_size=4)
    good = draw_mix(4, 16, 16, 0.8, 1.0, generator=_gen(1))
    view = cm.load(good, 16, 16)
    assert torch.equal(view, good) and view.data_ptr() == cm.table.data_ptr()
    small = cm.load(draw_mix(3, 16, 16, 0.8, 0.0, generator=_gen(2)), 16, 16)      # a smaller last batch: the first n rows
    assert tuple(small.shape) == (3, 8) and small.data_ptr() == cm.table.data_ptr() and torch.equal(cm.table[3], good[3])
    bad = []
    for col, row, value in [(0, 0, 4.0), (0, 0, -1.0), (0, 1, 3.0), (1, 0, 1.5), (1, 2, -0.1), (6, 0, 1.01), (6, 3, -1.0),
                            (4, 1, 17.0), (5, 1, 16.5), (2, 0, -1.0), (3, 2, -2.0)]:
        rows = good.clone()
        rows[row, col] = value
        bad.append((col, rows))
    rows = good.clone()
    rows[0, 0], rows[1, 0] = 1.0, 0.0                                            # 0 -> 1 -> 0 but 3 -> 0, 2 -> 1: not mutual
    bad.append((0, rows))
    words = {0: "partner", 1: "lam", 6: "weight", 2: "box", 3: "box", 4: "box", 5: "box"}
    for col, rows in bad:
        before = cm.table.clone()
        with pytest.raises(ValueError, match=words[col]):
            cm.load(rows, 16, 16)
        assert torch.equal(cm.table, before)
    with pytest.raises(ValueError, match="not mutual"):
        cm.load(bad[-1][1], 16, 16)
    with pytest.raises(ValueError, match="5 mix rows for a table of 4"):
        cm.load(R.identity_rows(5), 16, 16)


# ------------------------------------------------------------------ the float64 restatement
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("k", [1, 7, 249])
def test_ref64_loss_is_torchs_soft_target_cross_entropy(k, eps):
    g = _gen(k)
    n = 6
    z = (torch.randn(n, k, generator=g) * 4).float()
    y = torch.randint(0, k, (n,), generator=g)
    rows = R.identity_rows(n)
    rows[:, 0] = torch.tensor([5.0, 4.0, 2.0, 3.0, 1.0, 0.0])
    rows[:, 6] = torch.tensor([0.3, 0.8, 1.0, 0.0, 0.8, 0.3])
    ref = R.ref_softmax_ce_mix(z, y, rows, eps, 0.5)
    w, p = rows[:, 6].double()[:, None], rows[:, 0].long()
    target = w * F.one_hot(y, k).double() + (1 - w) * F.one_hot(y[p], k).double()
    zz = z.double().requires_grad_(True)
    want = F.cross_entropy(zz, target, label_smoothing=H.f32(eps))
    want.backward()
    want = want.detach()
    assert abs(float(ref["loss"]) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((ref["dl"] - zz.grad * 0.5).abs().max()) <= 1e-14
    assert bool((ref["a"] >= ref["dl"].abs()).all()) and float(ref["a_loss"]) >= abs(float(ref["loss"]))
    # identity rows (and rows None): the hard-label form of head_ref64
    hard = H.softmax_ce(z, y, 0.5)
    for r in (R.identity_rows(n), None):
        mine = R.ref_softmax_ce_mix(z, y, r, 0.0, 0.5)
        assert torch.equal(mine["dl"], hard["dl"]) and torch.equal(mine["a"], hard["a"]) and mine["correct"] == hard["correct"]
        assert float(mine["loss"]) == float(hard["loss"]) and float(mine["a_loss"]) == float(hard["a_loss"])
    if k > 1:
        smooth = R.ref_softmax_ce_mix(z, y, None, 0.1, 1.0)
        want = F.cross_entropy(z.double(), y, label_smoothing=H.f32(0.1))
        assert abs(float(smooth["loss"]) - float(want)) <= 1e-12 * abs(float(want))


def test_ref_mix_is_the_plain_expression():
    x = R.mix_input(4, 2, 3, 9, 11, torch.float32)
    rows = R.identity_rows(4)
    rows[0] = torch.tensor([3, 0.3, 0, 0, 0, 0, 0.3, 0])
    rows[3] = torch.tensor([0, 0.3, 0, 0, 0, 0, 0.3, 0])
    rows[1] = torch.tensor([2, 1.0, 2, 3, 6, 9, 0.8, 0])
    rows[2] = torch.tensor([1, 1.0, 2, 3, 6, 9, 0.8, 0])
    got = R.ref_mix(x, rows)
    lam = torch.tensor(0.3)
    assert torch.equal(got[0], lam * x[0] + (1 - lam) * x[3]) and torch.equal(got[3], lam * x[3] + (1 - lam) * x[0])
    want = x[1].clone()
    want[:, :, 2:6, 3:9] = x[2][:, :, 2:6, 3:9]
    assert torch.equal(got[1], want)
    # float64, every op rounded on its own: what the fp32 expression is on the CPU
    r64 = ((lam.double() * x[0].double()).float().double() + ((1 - lam).double() * x[3].double()).float().double()).float()
    assert torch.equal(got[0], r64)
    xb = x.to(torch.bfloat16)
    assert torch.equal(R.ref_mix(xb, rows), R.ref_mix(xb.float(), rows).to(torch.bfloat16))
    # the header's guard: a partner out of range or not mutual leaves both clips as they are
    for bad in (7.0, -1.0, 1.0):
        r = rows.clone()
        r[0, 0] = bad
        g = R.ref_mix(x, r)
        assert torch.equal(g[0], x[0]) and torch.equal(g[3], x[3]) and torch.equal(g[1], got[1])


# ------------------------------------------------------------------ the binding of include/sfk_mix.h
def test_mix_table_matches_its_header(lib, tmp_path):
    from video_classification_amd import _lib
    raw = open(os.path.join(ROOT, "include", "sfk_mix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(sfk_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.SIGNATURES_MIX) == ["sfk_clip_mix", "sfk_mix_abi_version", "sfk_softmax_ce_mix"]
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_V2, _lib.SIGNATURES_AUG, _lib.SIGNATURES_OPTIM, _lib.SIGNATURES_GROUPS):
        assert not set(names) & set(table)
    for n in names:
        assert hasattr(lib, n)
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES_MIX[n]), n
    assert lib.sfk_mix_abi_version() == _lib.MIX_ABI_VERSION == 1 == int(re.search(r"#define\s+SFK_MIX_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.MIX_ROW_FLOATS == 8 == int(re.search(r"#define\s+SFK_MIX_ROW_FLOATS\s+(\d+)", src).group(1))
    body = re.search(r"typedef struct \{(.*?)\} sfk_mix_desc;", src, flags=re.S).group(1)
    fields, sizes = [], {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "float": 4}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(3).replace("*", "").split(","):
            fields.append((nm.strip(), 8 if m.group(2) else sizes[m.group(1)]))
    assert [(f, ctypes.sizeof(t)) for f, t in _lib._MixDesc._fields_] == fields
    assert ctypes.sizeof(_lib._MixDesc) == 80 == _lib.new_mix_desc().struct_size
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfk_mix.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                    'sizeof(sfk_mix_desc), offsetof(sfk_mix_desc, n), offsetof(sfk_mix_desc, rows)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(_lib._MixDesc), _lib._MixDesc.n.offset, _lib._MixDesc.rows.offset]


def _good_mix(x, rows):
    from video_classification_amd import _lib
    d = _lib.new_mix_desc()
    d.dtype, d.x, d.rows = _lib.SFK_F32, x.data_ptr(), rows.data_ptr()
    d.n, d.t, d.c, d.h, d.w, d.c_off = 2, 3, 7, 16, 24, 0
    d.sn, d.st, d.sc, d.sh = 3 * 7 * 16 * 24, 7 * 16 * 24, 16 * 24, 24
    return d


def test_mix_rejects_bad_descriptors_on_the_host(lib):
    """every call here is refused before any launch (no GPU in this test)"""
    x, rows = torch.zeros(2 * 3 * 7 * 16 * 24), R.identity_rows(2)
    before = (x.clone(), rows.clone())
    B = ctypes.byref
    for field, value in [("struct_size", 8), ("struct_size", 76), ("struct_size", 88), ("x", None), ("rows", None), ("n", 0),
                         ("t", -1), ("c", 0), ("h", 0), ("w", -3), ("sn", -1), ("st", -5), ("sc", -1), ("sh", -24),
                         ("c_off", -1), ("dtype", 2), ("dtype", -1)]:
        d = _good_mix(x, rows)
        setattr(d, field, value)
        assert lib.sfk_clip_mix(B(d), None) == -1, (field, value)
    assert lib.sfk_clip_mix(None, None) == -1
    for fields in [dict(n=(1 << 23) + 1), dict(n=1 << 14, t=64, c=21, h=192, w=192), dict(t=1 << 12, c=21, h=1 << 12, w=64)]:
        d = _good_mix(x, rows)                            # more workgroups than the cap; a clip of more than 2^30 units
        for f, v in fields.items():
            setattr(d, f, v)
        assert lib.sfk_clip_mix(B(d), None) == -2, fields
    z, y, dl = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 5)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    F_ = lambda t: ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))
    ce = lib.sfk_softmax_ce_mix
    good = [F_(z), P(y), F_(rows), 0.1, 2, 5, 1.0, F_(dl), None, None, None, None]
    for i, value in [(0, None), (1, None), (4, 0), (4, -1), (5, 0), (5, -2), (3, 1.0), (3, -0.01), (3, 1.5), (3, float("nan"))]:
        args = list(good)
        args[i] = value
        assert ce(*args) == -1, (i, value)
    assert all(torch.equal(a, b) for a, b in zip(before, (x, rows))) and float(dl.abs().max()) == 0


# ------------------------------------------------------------------ the emulated backend and its mutants
def _mix_verdicts(be):
    vs = []
    for (h, w), layout, n, dtype in [((17, 19), "5of7_gap5", 6, torch.float32), ((32, 32), "7ch", 5, torch.bfloat16),
                                     ((17, 19), "21ch", 2, torch.float32), ((32, 32), "7ch", 1, torch.float32)]:
        vs += R.check_clip_mix(be, "cpu", h, w, layout, n, dtype)
    return vs


def _ce_verdicts(be):
    vs = []
    for case in [(7, 5, 0.1, "sd1"), (249, 5, 0.1, "sd40"), (257, 5, 0.0, "sd1"), (1000, 1, 0.1, "shift3e4"), (1, 5, 0.1, "equal"),
                 (249, 5, 0.1, "neginf"), (249, 5, 0.0, "neginf")]:
        vs += R.check_ce_mix(be, "cpu", case)
    return vs + R.check_ce_mix_correct(be, "cpu")


def test_emulated_backend_passes_the_checks_the_gpu_file_runs():
    be = EmuMixBackend()
    vs = _mix_verdicts(be) + _ce_verdicts(be)
    assert len(vs) > 300 and not H.failures(vs), H.failures(vs)[:5]


class _SecondMemberSeesTheMixedFirst(EmuMixBackend):
    def _mixed(self, clip, rows, c_off, c):
        out = clip.clone()
        p = R.partners(rows)
        for i in range(clip.shape[0]):                    # clip after clip, in place: the upper member reads the mixed lower one
            out[i] = R.ref_mix(out, rows, c_off, c)[i]
        return out


class _BoxOnOneMemberOnly(EmuMixBackend):
    def _mixed(self, clip, rows, c_off, c):
        r = rows.clone()
        p = R.partners(rows.cpu())
        for i in range(r.shape[0]):
            if int(p[i]) < i:
                r[i, 2:6] = 0.0
        out = R.ref_mix(clip, r, c_off, c)
        return out


class _WeightIgnored(EmuMixBackend):
    def _loss(self, lg, labels, rows, smoothing, gscale):
        ref = R.ref_softmax_ce_mix(lg, labels, rows, smoothing, gscale)
        r = None if rows is None else rows.clone()
        if r is not None:
            r[:, 6] = 1.0
        ref["dl"] = R.ref_softmax_ce_mix(lg, labels, r, smoothing, gscale)["dl"]
        return ref


class _NoSmoothingInDlogits(EmuMixBackend):
    def _loss(self, lg, labels, rows, smoothing, gscale):
        ref = R.ref_softmax_ce_mix(lg, labels, rows, smoothing, gscale)
        ref["dl"] = R.ref_softmax_ce_mix(lg, labels, rows, 0.0, gscale)["dl"]
        return ref


class _CorrectAlwaysAgainstY1(EmuMixBackend):
    def _loss(self, lg, labels, rows, smoothing, gscale):
        ref = R.ref_softmax_ce_mix(lg, labels, rows, smoothing, gscale)
        ref["correct"] = R.ref_softmax_ce_mix(lg, labels, None, smoothing, gscale)["correct"]
        return ref


@pytest.mark.parametrize("mutant,run,word", [
    (_SecondMemberSeesTheMixedFirst, _mix_verdicts, "clip_mix bits"), (_BoxOnOneMemberOnly, _mix_verdicts, "clip_mix bits"),
    (_WeightIgnored, _ce_verdicts, "dlogits"), (_NoSmoothingInDlogits, _ce_verdicts, "dlogits"),
    (_CorrectAlwaysAgainstY1, _ce_verdicts, "correct")])
def test_mutants_are_refused(mutant, run, word):
    bad = H.failures(run(mutant()))
    assert bad and all(word in v.name for v in bad), bad[:5]


# ------------------------------------------------------------------ the wiring
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
    cfg.MODEL.LR = 1e-3
    cfg.NUM_CPU = 0
    for k, v in model.items():
        setattr(cfg.MODEL, k, v)
    return cfg


MIX_ON = dict(LABEL_SMOOTHING=0.1, MIXUP_ALPHA=0.8, CUTMIX_ALPHA=1.0)


def test_config_defaults():
    from video_classification_amd.config import get_cfg
    m = get_cfg().MODEL
    assert (m.LABEL_SMOOTHING, m.MIXUP_ALPHA, m.CUTMIX_ALPHA, m.MIX_PROB, m.MIX_SWITCH_PROB, m.MIX_SEED) == (0.0, 0.0, 0.0, 1.0, 0.5, 0)
    assert v1.mix_settings(get_cfg()) == (0.0, None, 0)
    eps, draw, seed = v1.mix_settings(_cfg(MIX_SEED=3, **MIX_ON))
    assert (eps, seed) == (0.1, 3) and draw == dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)
    with pytest.raises(ValueError, match="LABEL_SMOOTHING"):
        v1.mix_settings(_cfg(LABEL_SMOOTHING=1.0))


def _v1_sets(cfg):
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True)
    te = v1.SyntheticChalearn(cfg, "test", num_videos=2, seed=2)
    return tr, te


def _spy(t, seen):
    prepare = t.mm.prepare_data

    def spy(batch):
        before = None
        if "mix" in batch:                                # the clip this batch would be without the entry, and the rows as drawn
            plain = {k: v for k, v in batch.items() if k != "mix"}
            before = prepare(plain)[0]
        x, y = prepare(batch)
        seen.append((batch.get("mix").clone() if "mix" in batch else None, before, x))
        return x, y
    t.mm.prepare_data = spy


def _cat(x):
    return x if isinstance(x, torch.Tensor) else torch.cat(list(x), dim=1)


@pytest.mark.parametrize("name", ["slowfast-LHand", "res3d"])
def test_v1_trainer_epoch_mixes_and_smooths(name):
    cfg = _cfg(name, **MIX_ON)
    tr, te = _v1_sets(cfg)
    be = EmuMixBackend()
    torch.manual_seed(0)
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    seen = []
    _spy(t, seen)
    be.launches.clear()
    loss, _ = t.train_epoch()
    assert math.isfinite(loss) and len(seen) == 2
    assert be.launches == ["clip_mix", "softmax_ce_mix"] * 2                      # one mix and one loss launch per step
    table = t.mm.clip_mix().table
    for rows, before, x in seen:
        assert tuple(rows.shape) == (2, 8) and rows[:, 0].tolist() == [1.0, 0.0]
        want = R.ref_mix(_cat(before).permute(0, 2, 1, 3, 4), rows).permute(0, 2, 1, 3, 4)
        assert torch.equal(_cat(x), want)
    assert not torch.equal(seen[0][0], seen[1][0])                               # the generator advances per step
    assert torch.equal(table, seen[1][0])                                         # one table, rewritten in place
    # the same seed and epoch: the same rows; another epoch: other rows
    again = draw_mix(2, 64, 64, generator=t._mix_generator(), **t.mix_draw)
    assert torch.equal(again, seen[0][0])
    t.epoch = 1
    assert not torch.equal(draw_mix(2, 64, 64, generator=t._mix_generator(), **t.mix_draw), again)


def test_v2_trainer_epoch_mixes_and_smooths_with_a_smaller_last_batch(tmp_path):
    cfg = _cfg("gesture-v2", **MIX_ON)
    cfg.CHALEARN.ROOT = str(tmp_path)
    tr = v2.SyntheticGesture(cfg, "train", num_videos=3, seed=1, h=48, w=64, min_box=8)
    te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    be = EmuMixBackend()
    t = v2.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    seen = []
    _spy(t, seen)
    be.launches.clear()
    loss, _ = t.train_epoch()
    assert math.isfinite(loss) and [tuple(s[0].shape) for s in seen] == [(2, 8), (1, 8)]
    assert be.launches == ["clip_mix", "softmax_ce_mix"] * 2
    assert seen[1][0].tolist() == [[0, 1, 0, 0, 0, 0, 1, 0]]                      # one clip: a self pair
    assert seen[1][0].data_ptr() != 0 and tuple(t.mm.clip_mix().table.shape) == (2, 8)
    for rows, before, x in seen:
        want = R.ref_mix(_cat(before).permute(0, 2, 1, 3, 4), rows).permute(0, 2, 1, 3, 4)
        assert torch.equal(_cat(x), want)
    assert not torch.equal(_cat(seen[0][2]), _cat(seen[0][1]))


def test_v2_float_batch_is_mixed_on_the_device_copy():
    g = _gen(2)
    mm = v2.ModelManager(_cfg("gesture-v2"), "cpu", EmuMixBackend())
    fb = {"rgb": torch.rand(2, 4, 3, 64, 64, generator=g), "uv": torch.rand(2, 4, 2, 64, 64, generator=g),
          "flow": torch.rand(2, 4, 2, 64, 64, generator=g), "label": torch.tensor([1, 5])}
    keep = {k: v.clone() for k, v in fb.items()}
    rows = draw_mix(2, 64, 64, 0.8, 0.0, generator=g)
    (s0, f0), _ = mm.prepare_data(fb)
    (s1, f1), _ = mm.prepare_data(dict(fb, mix=mm.clip_mix(2).load(rows, 64, 64)))
    assert all(torch.equal(fb[k], keep[k]) for k in fb)
    want = R.ref_mix(torch.cat([s0, f0], 1).permute(0, 2, 1, 3, 4), rows).permute(0, 2, 1, 3, 4)
    assert torch.equal(torch.cat([s1, f1], 1), want) and not torch.equal(s1, s0)


@pytest.mark.parametrize("name,channels", [("slowfast-LHand", 20), ("res3d", 5), ("res2d", 5)])
def test_v1_float_batch_is_mixed_on_a_copy_and_only_in_the_channels_the_model_reads(name, channels):
    g = _gen(3)
    be = EmuMixBackend()
    mm = v1.ModelManager(_cfg(name), "cpu", be)
    assert mm.mix_channels() == channels
    fb = {KEY: torch.randn(2, 4, 21, 64, 64, generator=g), "label": torch.tensor([0, 3])}
    keep = fb[KEY].clone()
    rows = draw_mix(2, 64, 64, 0.0, 1.0, generator=g)
    x0, _ = mm.prepare_data(fb)
    seen = []
    clip_mix = be.clip_mix
    be.clip_mix = lambda clip, table, c_off=0, c=None: (seen.append((tuple(clip.shape), c_off, c)), clip_mix(clip, table, c_off, c))[1]
    x1, _ = mm.prepare_data(dict(fb, mix=mm.clip_mix(2).load(rows, 64, 64)))
    assert torch.equal(fb[KEY], keep) and seen == [((2, 4, 21, 64, 64), 0, channels)]
    want = R.ref_mix(keep, rows)
    if name == "res2d":
        assert torch.equal(x1, want[:, :, :5]) and not torch.equal(x1, x0)
    else:
        assert torch.equal(_cat(x1), want.permute(0, 2, 1, 3, 4)[:, :channels]) and not torch.equal(_cat(x1), _cat(x0))


def test_resident_train_sets_are_mixed_too(tmp_path):
    """MODEL.RESIDENT_TRAIN with the stems reading the gathered float clip: the v1 set through _float_clip, the v2 set's
    'clip_v2' tensor in place"""
    cfg = _cfg("slowfast-LHand", RESIDENT_TRAIN=True, RESIDENT_GB=24 * 64 * 64 * 21 / 2 ** 30, **MIX_ON)
    tr = v1.SyntheticChalearn(cfg, "train", num_videos=4, seed=1, as_uint8=True, frames_per_video=(3, 8))
    te = v1.SyntheticChalearn(cfg, "test", num_videos=3, seed=2, pooled=True, frames_per_video=(3, 9))
    be = EmuMixBackend()
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    seen = []
    _spy(t, seen)
    be.launches.clear()
    assert math.isfinite(t.train_epoch()[0]) and len(seen) == 2
    assert be.launches == ["clip_mix", "softmax_ce_mix"] * 2
    for rows, before, x in seen:
        assert torch.equal(_cat(x), R.ref_mix(_cat(before).permute(0, 2, 1, 3, 4), rows).permute(0, 2, 1, 3, 4))
    g = _cfg("gesture-v2", RESIDENT_TRAIN=True, RESIDENT_GB=80 * 48 * 64 * 7 / 2 ** 30, **MIX_ON)
    g.CHALEARN.ROOT = str(tmp_path)
    gtr = v2.SyntheticGesture(g, "train", num_videos=4, seed=1, h=48, w=64, min_box=8, videos=True, frames_per_video=(3, 8))
    gte = v2.SyntheticGesture(g, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
    t = v2.Trainer(g, train_set=gtr, test_set=gte, device="cpu", backend=be)
    shapes = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (shapes.append((sorted(batch), tuple(batch["mix"].shape))), prepare(batch))[1]
    be.launches.clear()
    assert math.isfinite(t.train_epoch()[0])
    assert shapes == [(["clip_v2", "label", "mix"], (2, 8))] * 2 and be.launches == ["clip_mix", "softmax_ce_mix"] * 2


def test_label_smoothing_alone_changes_only_the_loss_launch():
    cfg = _cfg("res3d", LABEL_SMOOTHING=0.1)
    tr, te = _v1_sets(cfg)
    be = EmuMixBackend()
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    assert t.mix_draw is None and t.mm._mix is None
    be.launches.clear()
    assert math.isfinite(t.train_epoch()[0])
    assert be.launches == ["softmax_ce_mix"] * 2 and t.mm._mix is None


@pytest.mark.parametrize("which", ["v1", "v2"])
def test_defaults_record_the_parents_launches(which, tmp_path):
    """every key at its default: no ClipMix object, no mix launch, sfk_softmax_ce and never sfk_softmax_ce_mix; the
    engine is asked for the loss with the parent's five positional arguments"""
    cfg = _cfg("gesture-v2" if which == "v2" else "slowfast-LHand")
    if which == "v2":
        cfg.CHALEARN.ROOT = str(tmp_path)
        tr = v2.SyntheticGesture(cfg, "train", num_videos=3, seed=1, h=48, w=64, min_box=8)
        te = v2.SyntheticGesture(cfg, "test", num_videos=2, clips_per_video=(1, 2), seed=2, h=48, w=64, min_box=8)
        mod = v2
    else:
        (tr, te), mod = _v1_sets(cfg), v1
    be = EmuMixBackend()
    t = mod.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    asked = []
    loss_ops = t.model.engine.loss_ops
    t.model.engine.loss_ops = lambda *a, **kw: (asked.append((len(a), sorted(kw))), loss_ops(*a, **kw))[1]
    seen = []
    prepare = t.mm.prepare_data
    t.mm.prepare_data = lambda batch: (seen.append(sorted(batch)), prepare(batch))[1]
    be.launches.clear()
    assert math.isfinite(t.train_epoch()[0])
    assert be.launches == ["softmax_ce"] * 2 and t.mm._mix is None and t.step.label_smoothing == 0.0
    assert all("mix" not in keys for keys in seen) and asked and all(a == (5, []) for a in asked)


def test_mix_refuses_what_it_cannot_do():
    be = EmuMixBackend()
    # MODEL.U8_STEM: the stems read the uint8 frames, there is no float clip
    u8 = _cfg("slowfast-LHand", U8_STEM=True, **MIX_ON)
    tr, te = _v1_sets(u8)
    with pytest.raises(ValueError, match="U8_STEM.*no float clip.*'mix'"):
        v1.Trainer(u8, train_set=tr, test_set=te, device="cpu", backend=be).train_epoch()
    # MODEL.POOL_STEM on the resident route
    pool = _cfg("slowfast-LHand", POOL_STEM=True, RESIDENT_TRAIN=True, RESIDENT_GB=24 * 64 * 64 * 21 / 2 ** 30, **MIX_ON)
    ptr = v1.SyntheticChalearn(pool, "train", num_videos=4, seed=1, as_uint8=True, frames_per_video=(3, 8))
    pte = v1.SyntheticChalearn(pool, "test", num_videos=3, seed=2, pooled=True, frames_per_video=(3, 9))
    with pytest.raises(ValueError, match="POOL_STEM.*no float clip.*'mix'"):
        v1.Trainer(pool, train_set=ptr, test_set=pte, device="cpu", backend=be).train_epoch()
    # label smoothing alone needs no float clip: the pooled stems run with it
    pool.MODEL.MIXUP_ALPHA = pool.MODEL.CUTMIX_ALPHA = 0.0
    be.launches.clear()
    assert math.isfinite(v1.Trainer(pool, train_set=ptr, test_set=pte, device="cpu", backend=be).train_epoch()[0])
    assert be.launches == ["softmax_ce_mix"] * 2
    # res2d with the torch backend: host plumbing, no loss launch and no device kernels
    for keys in (dict(LABEL_SMOOTHING=0.1), dict(MIXUP_ALPHA=0.8), dict(CUTMIX_ALPHA=1.0)):
        res2d = _cfg("res2d", RES2D_BACKEND="torch", **keys)
        with pytest.raises(ValueError, match="LABEL_SMOOTHING / MIXUP_ALPHA / CUTMIX_ALPHA.*res2d.*torch"):
            v1.Trainer(res2d, train_set=tr, test_set=te, device="cpu", backend=be)
    mm = v1.ModelManager(_cfg("res2d", RES2D_BACKEND="torch"), "cpu", be)
    with pytest.raises(ValueError, match="'mix' entry needs MODEL.RES2D_BACKEND = 'engine'"):
        mm.prepare_data({KEY: torch.zeros(2, 4, 21, 64, 64), "label": torch.tensor([0, 1]), "mix": R.identity_rows(2)})


def test_train_step_cache_key_follows_the_table_address():
    cfg = _cfg("res3d")
    tr, te = _v1_sets(cfg)
    be = EmuMixBackend()
    t = v1.Trainer(cfg, train_set=tr, test_set=te, device="cpu", backend=be)
    step = v1.TrainStep(t.model.engine, lr=1e-3, label_smoothing=0.1)
    x, y = t.mm.prepare_data(next(iter(t.train_loader)))
    ta, tb = R.identity_rows(2), R.identity_rows(2)
    for table, entries in ((None, 1), (ta, 2), (ta, 2), (tb, 3), (None, 3)):
        step(x, None, y, mix=table)
        assert len(step._cache) == entries
    with pytest.raises(ValueError, match="label_smoothing"):
        v1.TrainStep(t.model.engine, lr=1e-3, label_smoothing=1.0)
