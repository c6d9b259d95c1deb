"""The engine's forward/backward SCHEDULE (engine.py) against the oracle's autograd, on CPU, with the C-ABI
contract restated in tests/emu_backend.py standing in for libsfk.  What this pins: buffer wiring, concat
elimination, residual/shortcut gradient routing, BN statistics flow, checkpoint key scheme and layout
conversion.  The kernels themselves are compared with the same restatement on the GPU box (test_gpu_*.py)."""
import pytest
import torch

from emu_backend import EmuBackend, keep_mask
from helpers import rel_err, rel_l2
from oracle import my_slowfast as o
from video_classification_amd import arch
from video_classification_amd.slowfast import SlowFast


def randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)
            elif ".norm" in k and k.endswith("weight"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif ".norm" in k and k.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.2)
            elif k.endswith("proj.weight"):
                v.copy_(torch.randn(v.shape, generator=g) * 0.05)


def make_models(ref_style, num_class=7, dtype=torch.float32, device="cpu", backend=None, depth=18):
    """depth 18 = one (projection) block per stage; depth 26 = two: adds the identity-shortcut blocks, whose output
    gradient is accumulated in place and masked by the pass that finishes it (sfk_conv_desc.out_relu_bits)"""
    torch.manual_seed(1234)   # the oracle's conv init draws from the global RNG
    if ref_style:
        spec = arch.ref_spec(num_class=num_class, depth=depth, head_pool_kernels=((2, 2, 2), (2, 2, 2)))
        om = o.mini_slowfast(num_class, ref_style=True, depth=depth)
    else:
        spec = arch.canonical_spec(num_class=num_class, depth=depth, head_pool_kernels=((2, 2, 2), (8, 2, 2)))
        om = o.mini_slowfast(num_class, ref_style=False, depth=depth)
    randomize(om, 3)
    m = SlowFast(spec, dtype=dtype, device=device, backend=backend if backend is not None else EmuBackend())
    m.load_state_dict(om.state_dict(), strict=True)
    return om, m


def make_inputs(ref_style, n=2):
    g = torch.Generator().manual_seed(5)
    if ref_style:
        clips = torch.randn(n, 4, 21, 64, 64, generator=g)          # dataset memory layout N,T,C,H,W
        return o.prepare_slowfast_data(clips)                      # strided NCTHW views, as train.py:136-140
    frames = torch.randn(n, 3, 8, 64, 64, generator=g)
    return o.pack_pathway(frames)


def oracle_train_step_with_engine_mask(om, eng, x, labels):
    """Oracle forward/backward in train mode with the ENGINE's counter-based dropout mask injected into the
    oracle's head (replaces nn.Dropout), so both sides see the same Bernoulli draw."""
    n = x[0].shape[0]
    seed = int(eng.drop_seed[0]) + 1                    # Engine.forward() bumps the seed before running
    c_s = eng.wiring.stages[3][0][-1].conv_c.geom.cout

    def pre_head(mod, inp):
        f = inp[0]                                      # (n, 2304, T', H', W')
        P = f[0, 0].numel()
        ks = torch.from_numpy(keep_mask(seed, n, c_s, 0, P, 0.5)).view(n, c_s, *f.shape[2:])
        kf = torch.from_numpy(keep_mask(seed, n, f.shape[1] - c_s, c_s, P, 0.5)).view(n, -1, *f.shape[2:])
        return (f * (torch.cat([ks, kf], 1).float() / 0.5),)

    saved = om.blocks[6].dropout
    om.blocks[6].dropout = torch.nn.Identity()
    h = om.blocks[6].register_forward_pre_hook(pre_head)
    om.train()
    y = om([t for t in x])
    loss = torch.nn.functional.cross_entropy(y, labels)
    for p in om.parameters():
        p.grad = None
    loss.backward()
    h.remove()
    om.blocks[6].dropout = saved
    return y.detach(), loss.detach()


def oracle_grad_noise(om, eng, x, labels, eps=1e-7):
    """How far the ORACLE's own parameter gradients move (relative L2, per key) when the input is perturbed by
    ~1 fp32 ulp.  Train-mode BN + ReLU + MaxPool make the gradient discontinuous (a near-zero pre-activation or a
    near-tie arg-max resolves differently), so this floor sits around 1e-2 for the mini model; a wiring error in
    the engine shows up as O(1)."""
    g0 = {k: p.grad.clone() for k, p in om.named_parameters() if p.grad is not None}
    gen = torch.Generator().manual_seed(99)
    xp = [t * (1 + eps * torch.randn(t.shape, generator=gen)) for t in x]
    seed_before = eng.drop_seed.clone()
    state_before = {k: v.clone() for k, v in om.state_dict().items()}   # BN running stats advance in train mode
    oracle_train_step_with_engine_mask(om, eng, xp, labels)
    om.load_state_dict(state_before)
    eng.drop_seed.copy_(seed_before)
    noise = {k: rel_l2(p.grad, g0[k]) for k, p in om.named_parameters() if p.grad is not None}
    for k, p in om.named_parameters():
        if p.grad is not None:
            p.grad = g0[k]
    return noise


def grad_tolerance(noise, k, floor=3e-2, cap=0.15):  # one flip costs ~1e-2 even when the probe saw none
    """N=2 mini batches: a single flipped ReLU / arg-max moves a narrow tensor's gradient by percents, hence the loose
    bound; the N=8 tests (grad_tolerance_n8) are the sharp ones."""
    return min(cap, max(floor, 4.0 * max(noise.values()), 4.0 * noise[k]))


def grad_tolerance_n8(noise, k, floor):
    """batch 8: one flipped decision moves a tensor by < 1e-2 (measured: worst 5e-3 at depth 18, 1.8e-2 at depth 26), so
    the bound is a few percent with NO cap -- one wrong tap of nine is 0.33, one wrong channel of 8 is 0.35."""
    return max(floor, 4.0 * noise[k])


LABELS8 = [1, 4, 0, 6, 2, 3, 5, 1]


def engine_grads_as_state_dict(eng):
    """Read the gradient arena through the checkpoint layout conversion (reference tensor shapes)."""
    keep = eng.P.data.clone()
    eng.P.data.copy_(eng.G)
    gsd = eng.state_dict()
    eng.P.data.copy_(keep)
    return gsd


@pytest.mark.parametrize("ref_style", [True, False], ids=["ref", "canonical"])
def test_state_dict_roundtrip_and_counts(ref_style):
    om, m = make_models(ref_style)
    sd_o, sd_m = om.state_dict(), m.state_dict()
    assert set(sd_m) == set(sd_o)
    for k in sd_o:
        assert tuple(sd_o[k].shape) == tuple(sd_m[k].shape), k
        assert torch.equal(sd_o[k].float(), sd_m[k].float().cpu()), k
    assert m.num_parameters() == sum(p.numel() for p in om.parameters())


def test_full_size_parameter_counts():
    # arena bookkeeping only (no kernels run): the three pinned counts of SURVEY.md section 8c
    from video_classification_amd.engine import Engine
    e = Engine(arch.canonical_spec(400), dtype=torch.float32, device="cpu", backend=EmuBackend())
    assert e.num_parameters() == 34_566_488
    e = Engine(arch.ref_spec(249), dtype=torch.float32, device="cpu", backend=EmuBackend())
    assert e.num_parameters() == 38_077_321 and e.num_parameters(live_only=True) == 34_052_161


@pytest.mark.parametrize("ref_style", [True, False], ids=["ref", "canonical"])
def test_eval_forward_matches_oracle(ref_style):
    om, m = make_models(ref_style)
    x = make_inputs(ref_style)
    om.eval(); m.eval()
    with torch.no_grad():
        want = om(list(x))
    got = m(list(x))
    assert got.shape == want.shape
    assert rel_err(got, want) < 1e-4


@pytest.mark.parametrize("ref_style,depth", [(True, 18), (False, 18), (True, 26), (False, 26)],
                         ids=["ref", "canonical", "ref-d26", "canonical-d26"])
def test_train_step_matches_oracle(ref_style, depth):
    om, m = make_models(ref_style, depth=depth)
    if depth == 26:   # block-final BN gammas are zero-initialised and randomize() redraws them; identity blocks are live
        assert any(b.branch1 is None for st in m.engine.wiring.stages for pw in st for b in pw)
    x = make_inputs(ref_style)
    m.train()
    eng = m.engine
    labels = torch.tensor([1, 4])
    y_o, loss_o = oracle_train_step_with_engine_mask(om, eng, x, labels)
    noise = oracle_grad_noise(om, eng, x, labels)

    y_m = m(list(x))
    loss_m = torch.nn.functional.cross_entropy(y_m, labels)
    loss_m.backward()
    assert rel_err(y_m.detach(), y_o) < 1e-4
    assert abs(float(loss_m.detach()) - float(loss_o)) < 1e-4
    assert m.arena.grad is not None and torch.equal(m.arena.grad, eng.G)

    gsd = engine_grads_as_state_dict(eng)
    for k, p in om.named_parameters():
        if ".residual." in k or ".res_unit." in k:
            assert p.grad is None                         # dead branches of the reference fusion get no gradient
            continue
        e = rel_l2(gsd[k].cpu(), p.grad)
        assert e < grad_tolerance(noise, k), (k, e, noise[k])
    # running statistics advanced exactly like nn.BatchNorm3d
    osd = om.state_dict()
    for L in eng.layers:
        nk = L.cb.norm_key
        assert rel_err(L.rm.cpu(), osd[nk + ".running_mean"]) < 1e-4, nk
        assert rel_err(L.rv.cpu(), osd[nk + ".running_var"]) < 1e-4, nk
        assert int(L.nbt[0]) == int(osd[nk + ".num_batches_tracked"])


@pytest.mark.parametrize("ref_style,depth", [(True, 18), (False, 18), (True, 26), (False, 26)],
                         ids=["ref", "canonical", "ref-d26", "canonical-d26"])
def test_train_step_gradients_batch8(ref_style, depth):
    """the sharp whole-model gradient check (see grad_tolerance_n8)"""
    om, m = make_models(ref_style, depth=depth)
    x = make_inputs(ref_style, n=8)
    labels = torch.tensor(LABELS8)
    m.train()
    eng = m.engine
    y_o, loss_o = oracle_train_step_with_engine_mask(om, eng, x, labels)
    noise = oracle_grad_noise(om, eng, x, labels)
    y_m = m(list(x))
    torch.nn.functional.cross_entropy(y_m, labels).backward()
    assert rel_err(y_m.detach(), y_o) < 1e-4
    gsd = engine_grads_as_state_dict(eng)
    for k, p in om.named_parameters():
        if p.grad is None:
            continue
        e = rel_l2(gsd[k], p.grad)
        assert e < grad_tolerance_n8(noise, k, 2e-2 if depth == 18 else 4e-2), (k, e, noise[k])


def test_load_state_dict_strictness():
    om, m = make_models(True)
    sd = om.state_dict()
    sd.pop("blocks.6.proj.bias")
    with pytest.raises(RuntimeError):
        m.load_state_dict(sd, strict=True)
    res = m.load_state_dict(sd, strict=False)
    assert res.missing_keys == ["blocks.6.proj.bias"]


# ------------------------------------------------------------------ the single-pathway `res3d` network (slow_r50)
def make_res3d(num_class=7, dtype=torch.float32, device="cpu", backend=None):
    from video_classification_amd.slowfast import slow_r50
    torch.manual_seed(4321)
    om = o.slow_r50(num_class, input_channels=5, depth=18, head_pool=(2, 2, 2))
    randomize(om, 5)
    m = slow_r50(num_class, 5, dtype=dtype, device=device, backend=backend if backend is not None else EmuBackend(),
                 depth=18, head_pool_kernel=(2, 2, 2))
    m.load_state_dict(om.state_dict(), strict=True)
    return om, m


def res3d_input(n=2):
    clips = torch.randn(n, 4, 5, 64, 64, generator=torch.Generator().manual_seed(8))    # dataset layout N,T,C,H,W
    return o.prepare_res3d_data(clips)


def oracle_res3d_train_step(om, eng, x, labels):
    """as oracle_train_step_with_engine_mask, for create_resnet's head (pool -> dropout -> proj, blocks[5])"""
    n = x.shape[0]
    seed = int(eng.drop_seed[0]) + 1
    head = om.blocks[5]

    class EngineMask(torch.nn.Module):
        def forward(self, f):
            P = f[0, 0].numel()
            k = torch.from_numpy(keep_mask(seed, n, f.shape[1], 0, P, 0.5)).view(n, f.shape[1], *f.shape[2:])
            return f * (k.float() / 0.5)
    saved, head.dropout = head.dropout, EngineMask()
    om.train()
    y = om(x)
    loss = torch.nn.functional.cross_entropy(y, labels)
    for p in om.parameters():
        p.grad = None
    loss.backward()
    head.dropout = saved
    return y.detach(), loss.detach()


def test_res3d_keys_counts_and_eval_forward():
    om, m = make_res3d()
    sd_o, sd_m = om.state_dict(), m.state_dict()
    assert set(sd_m) == set(sd_o) and "blocks.0.conv.weight" in sd_m and "blocks.5.proj.bias" in sd_m
    for k in sd_o:
        assert torch.equal(sd_o[k].float(), sd_m[k].float().cpu()), k
    x = res3d_input()
    om.eval(); m.eval()
    with torch.no_grad():
        want = om(x)
    assert rel_err(m(x), want) < 1e-4
    # full size: pytorchvideo's slow_r50 (3-channel stem) has 32,454,096 parameters
    from video_classification_amd.engine import Engine
    e = Engine(arch.slow_r50_spec(400, 3), dtype=torch.float32, device="cpu", backend=EmuBackend())
    assert e.num_parameters() == 32_454_096
    assert sum(p.numel() for p in o.slow_r50(400, 3).parameters()) == 32_454_096


def test_res3d_train_step_matches_oracle():
    om, m = make_res3d()
    x = res3d_input()
    m.train()
    eng = m.engine
    labels = torch.tensor([2, 5])
    y_o, loss_o = oracle_res3d_train_step(om, eng, x, labels)
    y_m = m(x)
    loss_m = torch.nn.functional.cross_entropy(y_m, labels)
    loss_m.backward()
    assert rel_err(y_m.detach(), y_o) < 1e-4 and abs(float(loss_m.detach()) - float(loss_o)) < 1e-4
    gsd = engine_grads_as_state_dict(eng)
    for k, p in om.named_parameters():
        assert rel_l2(gsd[k].cpu(), p.grad) < 3e-2, k
    osd = om.state_dict()
    for L in eng.layers:
        assert rel_err(L.rm.cpu(), osd[L.cb.norm_key + ".running_mean"]) < 1e-4
        assert rel_err(L.rv.cpu(), osd[L.cb.norm_key + ".running_var"]) < 1e-4


# ------------------------------------------------------------------ the fused TrainStep as ONE unit (train.py:225-231, k times)
def check_filter_copies(eng, P_before):
    """White box: the compute-precision filter copies the step just used are the casts / transposes of the master
    weights as they were BEFORE the step's Adam update (a stale data-gradient copy `St` would pass every forward check)."""
    cast = P_before.to(eng.dtype)
    for L in eng.layers:
        n = L.w_numel
        w = cast[L.w_off:L.w_off + n]
        if eng.dtype != torch.float32:                  # fp32: S aliases the master arena itself
            assert torch.equal(eng.S[L.w_off:L.w_off + n], w), L.cb.conv_key
        if L.needs_dgrad:
            want = w.view(L.eg.cout, L.eg.wtaps, L.eg.cin).permute(2, 1, 0).reshape(-1)
            assert torch.equal(eng.St[L.w_off:L.w_off + n], want), L.cb.conv_key


def run_k_steps(om, m, x, labels, k, lr, oracle_step=None, device="cpu"):
    """k optimisation steps of the product's fused TrainStep against k steps of the oracle (forward, mean CE,
    zero_grad, backward, Adam(lr) -- oracle.my_slowfast.train_step's sequence with the engine's dropout mask injected).
    Returns ([(loss_oracle, loss_engine)], {key: (cosine, norm ratio, max abs diff) of the weight UPDATE})."""
    from video_classification_amd.train import TrainStep
    oracle_step = oracle_step or oracle_train_step_with_engine_mask
    eng = m.engine
    opt = torch.optim.Adam(om.parameters(), lr=lr)
    step = TrainStep(eng, lr=lr, use_graph=False)
    before = {kk: v.clone() for kk, v in om.state_dict().items()}
    xs = x if isinstance(x, (list, tuple)) else [x, None]
    xd = [None if t is None else t.to(device) for t in xs]
    yd = labels.to(device)
    m.train()
    losses = []
    for _ in range(k):
        _, loss_o = oracle_step(om, eng, x, labels)      # zero_grad + backward inside
        opt.step()
        P_before = eng.P.data.clone()
        loss_m = float(step(xd[0], xd[1], yd))
        check_filter_copies(eng, P_before)
        losses.append((float(loss_o), loss_m))
    assert int(eng.adam_step[0]) == k
    sd_o, sd_m = om.state_dict(), m.state_dict()
    assert set(sd_o) == set(sd_m)
    upd = {}
    for kk in sd_o:
        a, b = sd_o[kk], sd_m[kk].cpu()
        if ".residual." in kk or ".res_unit." in kk:     # dead parameters: no gradient, Adam leaves them alone
            assert torch.equal(a, b), kk
            continue
        if kk.endswith("num_batches_tracked"):
            assert int(a) == int(b) == k, kk
            continue
        if kk.endswith(("running_mean", "running_var")):
            assert rel_err(b, a) < 2e-2, kk              # 1e-4 after ONE step (tests above); weights differ by 2*lr now
            continue
        uo, um = (a - before[kk]).flatten().double(), (b - before[kk]).flatten().double()
        cos = float(uo @ um / (uo.norm() * um.norm() + 1e-30))
        upd[kk] = (cos, float(um.norm() / uo.norm().clamp_min(1e-30)), float((uo - um).abs().max()), int(uo.numel()))
    return losses, upd


def assert_k_step_parity(losses, upd, lr, k, loss_rtol=2e-2, min_cos=0.8, med_cos=0.985):
    """Adam's first update is lr*sign(g): a gradient element whose sign differs (near-zero gradients of a discontinuous
    BN+ReLU+MaxPool net) moves its weight by 2*lr, so the UPDATE is compared by direction and size per tensor.  A wrong
    step count in the bias correction scales every update by up to 3.2x, a missing zero_grad or a stale filter copy
    turns the later updates -- all far outside these bounds (measured on the GPU, batch 8: worst tensor 0.908, median
    0.994 at depth 26)."""
    import numpy as np
    # step 1 is a pure forward of identical weights; from step 2 on the 2*lr differences of sign-flipped elements feed
    # back through a loss that moves by O(1) per step on these tiny batches (measured on the GPU: 1e-5, 1e-3, 1e-1)
    for i, (lo, lm) in enumerate(losses):
        tol = 1e-4 if i == 0 else (loss_rtol if i == 1 else 0.2)
        assert abs(lo - lm) <= tol * max(abs(lo), 1e-3), losses
    cosines = sorted(v[0] for v in upd.values())
    assert cosines[0] > min_cos and float(np.median(cosines)) > med_cos, (cosines[:5], float(np.median(cosines)))
    for kk, (cos, ratio, mx, numel) in upd.items():
        # (measured up to 1.055 on a stem norm at depth 26, batch 8; an 8-element BatchNorm vector moves by 12 % when ONE
        # of its sign-like Adam updates flips in one of the k steps: 0.883 seen on the fast stem's norm.bias)
        lo_, hi_ = (0.9, 1.1) if numel > 64 else (0.75, 1.33)
        assert lo_ < ratio < hi_, (kk, ratio, numel)
        assert mx <= 3.2 * lr * k * 2, (kk, mx)          # |m_hat / sqrt(v_hat)| <= (1-b1)/sqrt(1-b2) = 3.16 per step


@pytest.mark.parametrize("ref_style,depth", [(True, 18), (False, 18), (True, 26)], ids=["ref", "canonical", "ref-d26"])
def test_train_step_k_steps_match_oracle(ref_style, depth):
    om, m = make_models(ref_style, depth=depth)
    x = make_inputs(ref_style)
    losses, upd = run_k_steps(om, m, x, torch.tensor([1, 4]), k=3, lr=2e-4)
    assert_k_step_parity(losses, upd, 2e-4, 3)


def test_res3d_train_step_k_steps_match_oracle():
    om, m = make_res3d()
    losses, upd = run_k_steps(om, m, res3d_input(), torch.tensor([2, 5]), k=3, lr=2e-4,
                              oracle_step=oracle_res3d_train_step)
    assert_k_step_parity(losses, upd, 2e-4, 3)


def test_engine_options_defaults_typed_env_mapping_and_no_environment_reads(monkeypatch):
    """EngineOptions: the product defaults are the measured best (nothing experimental on), from_env maps every documented SFK_*
    variable onto exactly one field with the right type, and Engine() itself never looks at the environment."""
    import dataclasses
    from video_classification_amd.engine import Engine, EngineOptions
    d = EngineOptions()
    assert d.fuse_bn_bwd is False and d.deterministic_wgrad is False and d.ablate_kinds == frozenset()
    assert d.non_default() == {}
    fields = {f.name for f in dataclasses.fields(EngineOptions)}
    assert {fld for fld, _ in EngineOptions._ENV.values()} <= fields
    assert len({fld for fld, _ in EngineOptions._ENV.values()}) == len(EngineOptions._ENV)          # one variable per field
    assert {kind for _, kind in EngineOptions._ENV.values()} == {"1", "!0", "i"}
    env = {"SFK_WGWS": "1", "SFK_FUSE_BNB": "2", "SFK_WGRAD_LANES": "2", "SFK_TAIL_MAXC": "64", "SFK_TAIL": "0",
           "SFK_SPLIT_ADAM": "no", "SFK_UNRELATED": "7"}
    o = EngineOptions.from_env(env)
    assert o.non_default() == {"deterministic_wgrad": True, "wgrad_lanes": 2, "tail_max_c": 64, "fuse_tail": False}
    # an Engine built without options ignores the same variables in the process environment
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    eng = Engine(arch.ref_spec(7, depth=18), dtype=torch.float32, device="cpu", backend=EmuBackend())
    assert eng.options.non_default() == {}
