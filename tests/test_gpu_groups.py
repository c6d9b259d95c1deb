"""include/sfk_groups.h on an MI355X.  sfk_adam_groups / sfk_sgd_groups against the header's contract, bit for bit: for every
segment the result of sfk_adam_hp / sfk_sgd_hp on that slice (tests/groups_ref.py), over the counts of tests/optim_ref64.py and
just above the grid cap, segment tables with boundaries at 0, 1, 3, 4, 5, 1023..1025, count-1 and count, an all-covering group,
an empty table, alternating runs of 1..7 elements and about 1000 segments over three groups, with slices that miss 16-byte
alignment, both shadows, clipping on and off and every decay mode / SGD flavour; one case per kernel also element by element
against float64; sfk_grad_norm_groups against sfk_grad_norm on the zeroed copy; a captured launch replayed along the per-group
rows; the host-side rejections; and the segment tables Engine.param_segments makes for the depth-18 model.
tests/test_groups_cpu.py runs the same checks on the emulated backend and sees every mutation rejected."""
import pytest
import torch

import groups_ref as GR
import head_ref64 as H
import optim_ref64 as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from video_classification_amd._lib import HipBackend
    return HipBackend()


def report(vs):
    print()
    for v in H.failures(vs):
        print(f"  {v}")
    print(f"  {len(vs)} verdicts, worst error/bound {H.worst_of(vs):.3g}")
    assert not H.failures(vs), H.failures(vs)[:5]


@pytest.mark.parametrize("count", O.COUNTS)
def test_update_groups_meet_the_contract(hip, count):
    vs = []
    for name, segs, kernel, off, sh, clip, mode, nesterov, momentum in GR.update_case_table(count):
        for step0 in (0, 1, len(GR.LR_ROWS[0]) + 5):
            vs += GR.check_update_groups(hip, hip, DEV, kernel, count, segs, step0, off, sh, clip, mode, nesterov=nesterov,
                                         momentum=momentum, tag=name)
    report(vs)


def test_every_option_crossed_at_one_count(hip):
    count, vs = 1025, []
    segs = GR.seg_bounds(count)
    for off, sh, clip, mi in O.hp_cross_table():
        vs += GR.check_update_groups(hip, hip, DEV, "adam", count, segs, 1, off, sh, clip, O.MODES[mi])
        vs += GR.check_update_groups(hip, hip, DEV, "sgd", count, segs, 1, off, sh, clip, O.MODES[mi % 2], nesterov=bool(mi == 2))
        vs += GR.check_update_groups(hip, hip, DEV, "sgd", count, segs, 1, off, sh, clip, O.MODES[mi % 2], momentum=0.0)
    report(vs)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_update_groups_just_above_the_grid_cap(hip, kernel):
    """sfk_adam_hp's grid cap x 1024 + 5 elements: the all-covering group must be the bits of ONE _hp launch on the whole arena
    (that launch's second trip and scalar tail); 1000 segments with unaligned bounds make more than 16384 (segment, tile)
    pairs, one workgroup each; two short segments at the ends of a frozen arena"""
    count = O.BIG
    many = GR.seg_many(count)
    assert sum(((e - 1) >> 10) - (b >> 10) + 1 for b, e, _, _ in many) > 16384
    vs = GR.check_update_groups(hip, hip, DEV, kernel, count, GR.seg_all(count), 1, 0, H.BF16, True, "l2", nesterov=True, tag="all")
    vs += GR.check_update_groups(hip, hip, DEV, kernel, count, many, 2, 1, None, False,
                                 "decoupled" if kernel == "adam" else "l2", tag="many")
    vs += GR.check_update_groups(hip, hip, DEV, kernel, count, [(0, 5, 1, 1), (count - 1030, count - 1, 2, 0)], 1, 0, H.F32, False,
                                 "l2", tag="mostly frozen")
    report(vs)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_one_case_element_by_element_against_float64(hip, kernel):
    """optim_ref64.adam_hp_ref / sgd_hp_ref per segment under head_ref64.compare_p / ref64.compare as they stand"""
    vs = []
    for count in (1025, 4099):
        for name in ("bounds", "alternating"):
            vs += GR.check_update_groups(hip, hip, DEV, kernel, count, GR.tables_for(count)[name], 1, 1, H.BF16, True,
                                         "decoupled" if kernel == "adam" else "l2", nesterov=True, ref64=True, tag=name)
    vs += GR.check_update_groups(hip, hip, DEV, kernel, 4099, GR.seg_many(4099), 2, 0, None, False, "l2", ref64=True, tag="many")
    report(vs)


@pytest.mark.parametrize("count", O.COUNTS + [O.BIG])
def test_grad_norm_groups(hip, count):
    vs = []
    tables = GR.tables_for(count) if count != O.BIG else {"many": GR.seg_many(count), "all": GR.seg_all(count),
                                                          "edges": [(0, 5, 0, 0), (count - 1030, count - 1, 0, 0)], "empty": []}
    for name, segs in tables.items():
        for kind in (("randn", "nan_frozen", "inf_frozen", "nan", "inf") if count != O.BIG else ("randn", "nan_frozen")):
            for off in (0, 1):
                vs += GR.check_norm_groups(hip, hip, DEV, count, segs, kind, off, tag=name)
    report(vs)


def test_captured_launch_follows_the_per_group_rows_on_replay(hip):
    """one sfk_adam_groups launch captured on a single stream and replayed three times against three eager launches, bit for
    bit: every group's rate is read from its row by the device's step counter, not baked into the graph"""
    count = 4099
    segs = GR.seg_bounds(count)
    gen = torch.Generator(device=DEV).manual_seed(78)
    p0, g0, m0, v0, _ = H.adam_inputs(count, 1, gen)
    rows = torch.tensor(GR.LR_ROWS, dtype=torch.float32, device=DEV)
    assert all(len({r[k] for r in GR.LR_ROWS}) == 3 for k in range(3)) and all(len(set(r[:3])) == 3 for r in GR.LR_ROWS)
    coef = torch.tensor([O.COEF], device=DEV)
    table = hip.group_table(segs, GR.WDS, count, DEV)
    (b1, b2), eps = H.ADAM_BETAS, H.ADAM_EPS

    def state():
        return [x.clone() for x in (p0, g0, m0, v0)] + [torch.zeros(1, dtype=torch.int64, device=DEV)]

    def launch(s):
        p, g, m, v, step = s
        return hip.adam_groups(p, g, m, v, count, table, rows, b1, b2, eps, 0.5, step, None, decay_mode="decoupled", clip_coef=coef)
    eager = state()
    run = launch(eager)
    for _ in range(3):
        run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    replayed = state()
    run2 = launch(replayed)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run2(side.cuda_stream)                      # loads the code object outside the capture
    torch.cuda.synchronize()
    for x, x0 in zip(replayed, (p0, g0, m0, v0, torch.zeros(1, dtype=torch.int64, device=DEV))):
        x.copy_(x0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run2(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(replayed[4][0]) == int(eager[4][0]) == 3
    for a, b in zip(eager[:4], replayed[:4]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(eager[0], p0)


def test_host_side_rejections_launch_nothing(hip):
    from video_classification_amd._lib import SfkError
    n = 4096
    st = torch.cuda.current_stream().cuda_stream
    p, g, m, v = (torch.full((n,), 0.5, device=DEV) for _ in range(4))
    step = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    rows = torch.ones(3, 2, device=DEV)
    parts, out = torch.zeros(hip.grad_norm_parts(n), dtype=torch.float64, device=DEV), torch.zeros(2, device=DEV)
    good = [(0, 5, 0, 1), (5, 1030, 1, 0), (2000, n, 2, 1)]
    (b1, b2), eps = H.ADAM_BETAS, H.ADAM_EPS
    for segs in ([(5, 1030, 1, 0), (0, 5, 0, 1)], [(0, 8, 0, 0), (4, 12, 0, 0)], [(0, n + 1, 0, 0)], [(0, 8, 3, 0)], [(8, 8, 0, 0)],
                 [(2 * i, 2 * i + 1, 0, 0) for i in range(2049)]):
        with pytest.raises(SfkError):
            hip.group_table(segs, GR.WDS, n, DEV)

    def tampered(field, value, k=1):
        t = hip.group_table(good, GR.WDS, n, DEV)
        setattr(t.host[k], field, value)
        return t
    bad = [tampered("begin", 3), tampered("end", 2500), tampered("end", n + 8, k=2), tampered("group", 3), tampered("group", -1),
           tampered("tile0", 7), tampered("begin", 1030)]
    for t in bad:
        for make in (lambda: hip.adam_groups(p, g, m, v, n, t, rows, b1, b2, eps, 1.0, step, None, decay_mode="l2"),
                     lambda: hip.sgd_groups(p, g, m, n, t, rows, 0.9, 0.0, False, 1.0, step, None, decay_mode="l2")):
            with pytest.raises(SfkError, match="invalid"):
                make()(st)
    for t in bad[:3] + bad[-1:]:
        with pytest.raises(SfkError, match="invalid"):
            hip.grad_norm_groups(g, n, t, 1.0, 1.0, parts, out)(st)
    t = hip.group_table(good, GR.WDS, n, DEV)
    for kw in (dict(decay_mode=3), dict(decay_mode=-1)):
        with pytest.raises(SfkError, match="invalid"):
            hip.adam_groups(p, g, m, v, n, t, rows, b1, b2, eps, 1.0, step, None, **kw)(st)
    with pytest.raises(SfkError, match="invalid"):
        hip.sgd_groups(p, g, m, n, t, rows, 0.9, 0.0, False, 1.0, step, None, decay_mode="decoupled")(st)
    with pytest.raises(SfkError, match="invalid"):
        hip.grad_norm_groups(g, n, t, 1.0, -1.0, parts, out)(st)
    torch.cuda.synchronize()
    assert int(step[0]) == 3 and all(bool((x == 0.5).all()) for x in (p, g, m, v)) and not out.any() and not parts.any()


# ------------------------------------------------------------------ the segment tables of a real model
def _mini():
    from video_classification_amd import arch
    from video_classification_amd.slowfast import SlowFast
    spec = arch.ref_spec(num_class=7, input_channels=(5, 2), depth=18, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
    return SlowFast(spec, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_engine_segment_tables_meet_the_contract(hip, kernel):
    """Engine.param_segments of the depth-18 SlowFast (10.8 M elements, every tensor boundary of a real arena): a frozen prefix
    with a 0.1x group, a frozen mid-stage with two groups, everything frozen but the fresh tensors of a pretrained load -- each
    table through the grouped launch against the _hp launches on its slices, and through the grouped norm"""
    eng = _mini().engine
    n = eng.arena_numel
    eng.fresh_keys = {k for k, _, _ in eng.param_tensors() if k.startswith(("blocks.0.multipathway_blocks", "blocks.6."))}
    tables = {
        "frozen prefix": eng.param_segments(["blocks.4."], ["blocks.0.", "blocks.1."], "weights"),
        "frozen mid-stage": eng.param_segments(["blocks.4.", "blocks.6."], ["blocks.2."], "all"),
        "@pretrained frozen": eng.param_segments(["blocks.6."], ["@pretrained"], "weights"),
    }
    vs = []
    for i, (name, segs) in enumerate(tables.items()):
        assert 1 < len(segs) <= 2048 and 0 < sum(e - b for b, e, _, _ in segs) < n, name
        vs += GR.check_update_groups(hip, hip, DEV, kernel, n, segs, 1 + i, 0, (None, H.BF16, H.F32)[i], i % 2 == 0,
                                     ("decoupled" if kernel == "adam" else "l2", "l2", "none")[i], nesterov=i == 1, tag=name)
        vs += GR.check_norm_groups(hip, hip, DEV, n, segs, ("randn", "nan_frozen", "inf")[i], 0, tag=name)
    report(vs)
