"""Training loop with the reference's surface (train.py): ``ModelManager(cfg)``, ``Trainer(cfg)``, ``.train()``,
``.train_epoch()``, ``.run_eval(loader) -> {'ps','t','acc','sv'}``, ``.save_ckpt/.load_ckpt``.

What differs from /root/reference/train.py, and why:
  * the step (forward, CrossEntropyLoss, zero_grad, backward, Adam -- train.py:225-231) is ONE flat schedule of
    libsfk kernels (``TrainStep``), optionally replayed as a hipGraph; loss and accuracy are accumulated on the
    device, so there is no ``.item()`` sync per step (train.py:236) -- they are read once per epoch;
  * N>1: one process per GPU; loaders the Trainer builds itself (from ``train_set`` / ``test_set`` or the reference's
    dataset) shard one shuffled epoch over the ranks (``dist.EpochShardSampler``) and the test videos round-robin
    (``dist.VideoShardSampler``, scores gathered to every rank); ``TrainStep`` all-reduces the gradient arena over RCCL
    while backward is still running (dist.py); rank 0 writes checkpoints.  Loaders that are INJECTED are used as they are
    (the caller shards them, or every rank sees everything).  The reference is single-GPU;
  * datasets are injected (``train_loader`` / ``test_loader``) or built from the reference's own
    ``ChalearnVideoDataset`` when that module is importable; items keep its contract: a dict
    {cfg.MODEL.R3D_INPUT: (T,21,S,S) float32, 'label': int} (lists of such dicts for the test set); the uint8 transport
    and the pooled test videos (``ChalearnVideoFramesU8``) are this engine's additions (input_pipeline.py).
"""
from __future__ import annotations

import contextlib
import glob
import os
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np
import torch
import torch.utils.data
from torch.utils.data.dataloader import default_collate

from . import dist as sdist
from .config import crop_resize_dict
from .engine import Engine
from .input_pipeline import STEM_CLIPS, h2d, is_pool_clips
from .optim import Optimizer
from .slowfast import init_my_slowfast


class TrainStep:
    """One optimisation step on one rank: forward -> mean cross-entropy -> backward -> (all-reduce) -> Adam.

    Default execution is eager on four HIP streams (engine.OpList lanes: slow pathway / trunk, fast pathway, one
    filter-gradient lane per pathway); the same schedule captured into ONE hipGraph replays its branches one after the
    other on this ROCm (round 1: 51.7 against 46.5 ms for two eager lanes), so ``use_graph=True`` is kept only for the
    lowest host load.  Every switch comes from ``engine.options`` (engine.EngineOptions); nothing here reads the environment."""

    def __init__(self, engine: Engine, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, use_graph: bool = False,
                 reducer: Optional[sdist.GradReducer] = None, overlap_segments: int = 6, optimizer: str = "adam",
                 momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False, lr_table=None,
                 weight_decay: float = 0.0, decay_mode: str = "none", decay_scope: str = "weights",
                 clip_grad_norm: float = 0.0, label_smoothing: float = 0.0, ema_decay: float = 0.0, ema_warmup: bool = False,
                 param_groups=(), freeze=(), trunk: Optional["torch.cuda.Stream"] = None):
        """optimizer 'adam' (train.py:182: lr, betas, eps) or 'sgd' (the v2 trainer, new_feature_test.py:832: lr, momentum,
        dampening, nesterov; one sfk_sgd launch over the arena, never split beside the last kernel).

        lr_table, weight_decay, decay_mode, decay_scope, clip_grad_norm: at their defaults the step issues exactly the
        launches above (sfk_adam / sfk_sgd with `lr` by value).  Otherwise the optimizer launch is sfk_adam_hp / sfk_sgd_hp
        (include/sfk_optim.h): lr_table (a sequence of per-step rates, see lr_schedule; None = `lr` at every step) goes to
        the device once and step s of THIS optimizer reads entry min(s, len) - 1 with the counter the launch keeps on the
        device, so a replayed graph follows the schedule; decay_mode 'none' | 'l2' (torch's Adam / SGD weight_decay) |
        'decoupled' (AdamW; Adam only) over decay_scope 'weights' (conv filters and the FC weight) | 'all'; clip_grad_norm
        > 0 runs sfk_grad_norm over the finished (reduced) gradients before one optimizer launch -- clip_grad_norm_(max_norm)
        -- and leaves (norm, coefficient) in self.grad_norm.  The optimizer state and the step count are not checkpointed
        (as in the reference), so a resumed run starts the table again.

        label_smoothing in [0, 1) and the ``mix`` table of a call (include/sfk_mix.h: two labels with a weight per clip): at
        0 and None the loss launch is sfk_softmax_ce as ever; otherwise the one sfk_softmax_ce_mix launch takes its place
        and nothing else of the step changes.

        ema_decay in [0, 1), ema_warmup (include/sfk_ema.h, ema.WeightEma): at 0 self.ema is None and the step issues exactly
        the launches above.  Otherwise one sfk_ema_update launch follows the step's last optimizer launch on the trunk: the
        average of the arena and of the BatchNorm running statistics, with its own step counter on the device.  With world >
        1 every rank averages its own identical copy; nothing is communicated.  The average is not checkpointed separately:
        self.ema.applied() evaluates and saves it.  Eager steps only: with use_graph the keyword is refused (DESIGN.md
        section 20 -- the captured step with the launch in it ended its capture in a host segmentation fault on the GPU, the
        cause is not known, and the captured route was taken out).

        param_groups, freeze (include/sfk_groups.h): both empty, the step issues exactly the launches
        above.  param_groups is a sequence of (selector, lr_mult) or (selector, lr_mult, wd_mult) in priority order, freeze a
        sequence of selectors; a selector is a state_dict() key prefix ('blocks.1.'), '@fresh' or '@pretrained' (the keys a
        pretrained load left untouched / filled); the first match wins and freeze beats groups.  The optimizer launch is then
        sfk_adam_groups / sfk_sgd_groups: group j's rate at step s is lr_table[s] * lr_mult_j, its decay weight_decay *
        wd_mult_j, a frozen tensor keeps its bits (moments included) and its gradient does not count in the clipped norm.  The
        engine's train plans are built for the frozen set (Engine.set_frozen): no filter-gradient launch whose only output
        is a frozen filter's gradient, and no backward below the last unit that holds a trainable parameter.  The forward is
        not pruned: frozen BatchNorm layers still normalise with batch statistics and update their running ones, as torch does
        for requires_grad = False under .train().  The frozen set is the ENGINE's: a TrainStep with another set on the same
        engine re-sets it, and a step that finds another step's set when it is called puts its own back first (the train plan
        is rebuilt, so alternating two such steps rebuilds a plan per switch) -- a step never runs on plans pruned for another
        set.  Eager steps only: with use_graph the keywords are refused, as ema_decay is
        and for the same reason (the captured grouped step ended its capture in the same host segmentation fault)."""
        self.eng = engine
        ema_decay = float(ema_decay)
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        param_groups, freeze = tuple(param_groups), tuple(freeze)
        captured = use_graph and not (reducer is not None and reducer.active) and engine.device.type == "cuda"
        if captured and (param_groups or freeze):        # before any state, table or plan exists
            raise ValueError("param_groups / freeze need an eager step: the captured step (use_graph=True) with the "
                             "sfk_adam_groups / sfk_sgd_groups launch in it is not offered (DESIGN.md section 18)")
        opt = self.opt = Optimizer(engine, optimizer, lr, betas, eps, momentum, dampening, nesterov, lr_table, weight_decay,
                                   decay_mode, decay_scope, clip_grad_norm, param_groups, freeze)   # validates; allocates no state
        self.last_lrs = opt.last_lrs
        # the train plans are built for this step's frozen set (no launch for a frozen filter's gradient, no backward below the
        # last trainable unit); a step with another set on the same engine re-sets it, which drops the cached train plans
        self.freeze = freeze
        self._frozen = engine.frozen_param_keys(freeze) if (freeze or engine.frozen_keys) else frozenset()
        if self._frozen != engine.frozen_keys:
            engine.set_frozen(freeze)
        self.optimizer, self.momentum, self.hp, self.lr_table = opt.optimizer, opt.momentum, opt.hp, opt.lr_table
        self.decay_mode, self.clip_grad_norm, self.last_lr = opt.decay_mode, opt.clip_grad_norm, opt.last_lr
        self.reducer = reducer
        self.world = reducer.world if reducer is not None else 1
        self.segmented = reducer is not None and reducer.active     # cut backward into segments and exchange them as they finish
        if self.segmented:
            # three compute lanes + the collective's own stream = the four hardware queues a process gets (dist.GradReducer);
            # measured only with the single-GPU stand-in (dist.LoopbackReducer), never on RCCL: options.dist_wgrad_one_lane = False
            # keeps the four compute lanes for an A/B on a multi-GPU node
            engine.wgrad_one_lane = engine.options.dist_wgrad_one_lane or engine.wgrad_one_lane
        self.use_graph = use_graph and not self.segmented and engine.device.type == "cuda"
        self.ema = None
        if ema_decay > 0:
            if self.use_graph:
                raise ValueError("ema_decay > 0 needs an eager step: the captured step (use_graph=True) with the sfk_ema_update "
                                 "launch in it is not offered (DESIGN.md section 20)")
            from .ema import WeightEma
            self.ema = WeightEma(engine, ema_decay, ema_warmup)
        self.overlap_segments = overlap_segments
        dev = engine.device
        self.loss = torch.zeros(1, device=dev)            # mean loss of the last step
        self.loss_sum = torch.zeros(1, device=dev)        # running sums since reset_meters()
        self.correct = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps = 0
        self._cache = {}
        # The trunk (lane 0: slow pathway, head, loss, optimiser) is the longest dependency chain of the step; it runs on a
        # HIGH-priority stream of its own so that its next kernel gets CUs ahead of the filter-gradient lanes' backlog
        # (measured +0.8 % clips/s).  The caller's stream waits for the step as before.
        self._trunk = None
        # trunk: a stream to use for it instead of a new one (steps that take turns on one engine share one: every new stream
        # takes another of the process's few hardware queues, and a trunk that shares a queue with a lane serialises with it)
        if dev.type == "cuda" and not self.use_graph and engine.options.trunk_priority:
            self._trunk = trunk if trunk is not None else torch.cuda.Stream(dev, priority=-1)
        self.trunk = self._trunk

    def reset_meters(self):
        self.loss_sum.zero_()
        self.correct.zero_()
        self.steps = 0

    grad_norm = property(lambda self: self.opt.grad_norm, doc="device float32[2] (norm, coefficient) of the last step; None "
                         "until a clipped step has been built")

    def _build(self, pl, labels, mix=None):
        eng, opt = self.eng, self.opt
        gscale = self.reducer.grad_scale if self.reducer is not None else 1.0
        if self.label_smoothing == 0.0 and mix is None:
            loss = eng.loss_ops(pl, labels, self.loss, self.loss_sum, self.correct)
        else:
            loss = eng.loss_ops(pl, labels, self.loss, self.loss_sum, self.correct, label_smoothing=self.label_smoothing, mix=mix)
        ops = dict(
            loss=loss,
            zero_loss=eng.be.fill_zero(self.loss),
            zero_grad=eng.be.fill_zero(eng.G),
        )
        if opt.clip_grad_norm > 0:
            ops["grad_norm"] = opt.norm_ops(gscale)       # runs after the whole backward, so a clipped step is never split
        ops["adam"] = opt.update_ops(gscale)              # the optimiser launch, Adam or SGD (the key bench.py's profiler reads)
        # the optimiser beside the last kernel of the step (engine.Plan.tail_cut): eager four-lane single-rank Adam steps only.
        # Not segmented, so the reducer's world, if there is one, is 1 and gscale is 1.
        if (opt.can_split and pl.tail_cut is not None and not self.segmented and not self.use_graph and eng.two_streams
                and eng.device.type == "cuda" and eng.options.split_adam):
            ops["adam_main"], ops["adam_tail"], self._set_tail = opt.split_ops(pl.tail_cut[1], gscale)
        if self.ema is not None:
            ops["ema"] = self.ema.update_ops()            # after the step's last optimizer launch, on the trunk
        return ops

    def _eager(self, pl, ops):
        eng = self.eng
        st = eng._stream()
        eng.drop_seed.add_(1)
        eng._run_lanes(pl.fwd)
        ops["zero_loss"](st)
        ops["loss"](st)
        ops["zero_grad"](st)
        if "adam_main" in ops:
            # everything but the fast stem's filter gradient; the trunk joins the other lanes as they stand, updates the
            # arena above the stems' filters while that last kernel runs on the fast pathway's lane, then the rest
            i_wg = pl.tail_cut[0]
            eng._run_lanes(pl.bwd, 0, i_wg)
            lanes = eng.lane_streams()
            for s_ in lanes[1:]:
                ev = torch.cuda.Event()
                ev.record(s_)
                lanes[0].wait_event(ev)
            ops["adam_main"](st)
            self._set_tail()                  # tail counter = step - 1, in the trunk's idle time (the tail launch increments it)
            eng._run_lanes(pl.bwd, i_wg)
            ops["adam_tail"](st)
            if "ema" in ops:
                ops["ema"](st)
            return
        if not self.segmented:
            eng._run_lanes(pl.bwd)
        else:
            self.reducer.begin()
            lanes = eng.lane_streams()
            issue = lanes[2] if len(lanes) > 2 else None     # the filter-gradient lane enqueues the buckets (no relay stream)
            for a, b, ranges in pl.grad_segments(self.overlap_segments):
                eng._run_lanes(pl.bwd, a, b)          # the pathway lanes and the filter-gradient lane, as the single-rank step
                self.reducer.reduce(ranges, lanes, issue_on=issue)
            self.reducer.finish()
        if "grad_norm" in ops:
            ops["grad_norm"](st)
        ops["adam"](st)
        if "ema" in ops:
            ops["ema"](st)

    def __call__(self, x_slow, x_fast, labels, slow_t_index=None, mix=None) -> torch.Tensor:
        """mix: None, or the (N, 8) float32 device table of the batch's mix rows (input_pipeline.ClipMix.load): the loss takes
        its soft target from it.  Its CONTENTS are read when the launch runs; its address is part of the cache key."""
        eng = self.eng
        if eng.frozen_keys != self._frozen:  # another TrainStep set the engine's frozen set since: this step's plans are gone
            eng.set_frozen(self.freeze)
        x_slow = eng.input_view(x_slow)      # res2d: the (N, C, T, H, W) view of its stacked-frames input; else x as it is
        pl = eng._plan_for(x_slow, x_fast, slow_t_index, True)
        if mix is not None:
            assert mix.dtype == torch.float32 and mix.is_contiguous() and tuple(mix.shape) == (labels.shape[0], 8), tuple(mix.shape)
        key = (pl.serial, labels.data_ptr(), pl.graph_epoch) + (() if mix is None else (mix.data_ptr(),))
        ent = self._cache.get(key)
        if ent is None:
            if len(self._cache) > 4:
                self._cache.clear()
            ent = {"ops": self._build(pl, labels, mix), "graph": None, "calls": 0, "labels": labels, "mix": mix}
            self._cache[key] = ent
        ent["calls"] += 1
        if not self.use_graph:
            if self._trunk is not None:
                cur = torch.cuda.current_stream(eng.device)
                self._trunk.wait_stream(cur)
                with torch.cuda.stream(self._trunk):
                    self._eager(pl, ent["ops"])
                cur.wait_stream(self._trunk)
            else:
                self._eager(pl, ent["ops"])
        elif ent["graph"] is not None:
            ent["graph"].replay()
        elif ent["calls"] < 2:
            self._eager(pl, ent["ops"])      # first call: eager (loads code objects, settles allocations)
        else:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._eager(pl, ent["ops"])
            ent["graph"] = g
            g.replay()
        self.steps += 1
        return self.loss


def mix_settings(cfg):
    """MODEL.LABEL_SMOOTHING and the MODEL.MIX* keys: (label_smoothing, draw_mix keywords | None, seed).  The keywords are
    None when both alphas are 0: no table is drawn, no clip is mixed."""
    m = cfg.MODEL
    eps = float(m.get("LABEL_SMOOTHING", 0.0))
    mixup, cutmix = float(m.get("MIXUP_ALPHA", 0.0)), float(m.get("CUTMIX_ALPHA", 0.0))
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"MODEL.LABEL_SMOOTHING must be in [0, 1), got {eps}")
    if mixup < 0 or cutmix < 0:
        raise ValueError(f"MODEL.MIXUP_ALPHA / MODEL.CUTMIX_ALPHA must be >= 0, got {mixup} / {cutmix}")
    draw = None
    if mixup > 0 or cutmix > 0:
        draw = dict(mixup_alpha=mixup, cutmix_alpha=cutmix, prob=float(m.get("MIX_PROB", 1.0)),
                    switch_prob=float(m.get("MIX_SWITCH_PROB", 0.5)))
    return eps, draw, int(m.get("MIX_SEED", 0))


def ema_settings(cfg):
    """MODEL.EMA_DECAY, EMA_WARMUP, EMA_EVAL: (decay, warmup, 'ema' | 'live' | 'both')"""
    m = cfg.MODEL
    decay, which = float(m.get("EMA_DECAY", 0.0)), str(m.get("EMA_EVAL", "ema"))
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"MODEL.EMA_DECAY must be in [0, 1), got {decay}")
    if which not in ("ema", "live", "both"):
        raise ValueError(f"MODEL.EMA_EVAL must be 'ema', 'live' or 'both', got {which!r}")
    return decay, bool(m.get("EMA_WARMUP", False)), which


def jitter_ranges(cfg):
    """MODEL.COLOR_JITTER on: the (brightness, contrast, saturation, hue) ranges of MODEL.JITTER_*; off: None"""
    m = cfg.MODEL
    if not bool(m.get("COLOR_JITTER", False)):
        return None
    return (float(m.get("JITTER_BRIGHTNESS", 0.5)), float(m.get("JITTER_CONTRAST", 0.3)),
            float(m.get("JITTER_SATURATION", 0.2)), float(m.get("JITTER_HUE", 0.1)))


def affine_ranges(cfg):
    """MODEL.AFFINE on: (degrees, (scale lo, scale hi), shear, flip) of MODEL.AFFINE_*, ``input_pipeline.draw_affine``'s
    arguments; off: None"""
    m = cfg.MODEL
    if not bool(m.get("AFFINE", False)):
        return None
    lo, hi = m.get("AFFINE_SCALE", (0.85, 1.15))
    return (float(m.get("AFFINE_DEGREES", 10.0)), (float(lo), float(hi)), float(m.get("AFFINE_SHEAR", 0.0)),
            float(m.get("AFFINE_FLIP", 0.0)))


def draw_crop_or_warp(cfg, size: int, generator=None) -> tuple:
    """('crop', (2,) int32) of RandomCrop(size, padding = size // 10), or, under MODEL.AFFINE, ('warp', (6,) float32) of
    ``draw_affine`` -- whose first two draws are the crop's, so everything drawn after it keeps its stream position"""
    from .input_pipeline import draw_affine, draw_crop_offsets
    ranges = affine_ranges(cfg)
    if ranges is None:
        return "crop", draw_crop_offsets(1, size // 10, generator)[0]
    return "warp", draw_affine(1, size, size // 10, *ranges, generator=generator)[0]


class ModelManager:
    """Name -> (init_model, prepare_data), as reference train.py:39-60.  'slowfast*' and 'res3d' (SURVEY.md section
    8f-4: hub slow_r50 with a 5-channel stem, train.py:79-89 / (deprecated)/train_3dresnet.py:47-51) run on this
    engine; 'res2d' (torchvision's 2-D ResNet-50 over T*C stacked frames, train.py:64-76) is host plumbing
    (res2d.py: BASELINE config 1, "CPU reference path, no GPU") unless MODEL.RES2D_BACKEND = 'engine', which builds the
    same network on the engine (slowfast.resnet50_2d_engine, MODEL.DTYPE).  MODEL.ARCH = 'canonical8x8' swaps the SlowFast
    geometry for the hub model's ((deprecated)/(torchvideo)train.py:44-71,249)."""

    def __init__(self, cfg, device="cuda", backend=None):
        self.cfg, self.device, self.backend = cfg, device, backend
        self._pre = None
        self._lut = None
        self._jit = None
        self._mix = None
        self._resize = None
        name = cfg.MODEL.NAME
        self.arch = str(cfg.MODEL.get("ARCH", "ref")).lower()
        if self.arch not in ("ref", "canonical8x8"):
            raise ValueError(f"MODEL.ARCH={self.arch!r}: 'ref' or 'canonical8x8'")
        if name == "res2d":
            self.init_model = self._init_res2d_model
            self.prepare_data = self._prepare_res2d_data
        elif name == "res3d":
            self.init_model = self._init_res3d_model
            self.prepare_data = self._prepare_res3d_data
        elif "slowfast" in name:
            if self.arch == "canonical8x8":
                self.init_model = self._init_canonical_model
                self.prepare_data = self._prepare_canonical_data
            else:
                self.init_model = self._init_slowfast_model
                self.prepare_data = self._prepare_slowfast_data
        else:
            raise NotImplementedError()

    def _h2d(self, t: torch.Tensor) -> torch.Tensor:
        """host -> device through PINNED memory, so the copy is a DMA that overlaps the previous step's kernels (a
        pageable source makes `non_blocking=True` a synchronous staged copy: train.py:127's 1.5 GB batch would stall the
        host for its whole duration).  Loaders built by the Trainer already pin (pin_memory=True)."""
        return h2d(t, self.device)

    # ---- the uint8 transport: a batch carrying <R3D_INPUT>_u8 (N,T,S,S,P uint8 HWC frames, P >= the channels read, optional
    #      `crop` (N,2)) instead of the float32 tensor.  MODEL.U8_STEM False: DevicePreprocess writes the normalised, cropped
    #      float clip on the device and the stems read its views; True: the stems read the frames themselves (U8Clip).
    def _u8_key(self, batch) -> Optional[str]:
        key = self.cfg.MODEL.R3D_INPUT + "_u8"
        return key if key in batch else None

    # ---- the raw transport: a batch carrying <R3D_INPUT>_raw (the clips' crops at their native sizes, HWC bytes end to end)
    #      and raw_hw (N,T,2) -- collate_raw's -- instead of the resized frames.  PadResize writes the (N,T,S,S,21) uint8
    #      frames on the device and the batch goes on as a <R3D_INPUT>_u8 batch whose frames are already there.
    def _resized(self, batch):
        key = self.cfg.MODEL.R3D_INPUT
        if key + "_raw" not in batch:
            return batch
        from .input_pipeline import PadResize, raw_offsets
        size = crop_resize_dict[key]
        if self._resize is None:
            self._resize = PadResize(size, self.device, self.backend)
        hw = torch.as_tensor(batch["raw_hw"])
        assert hw.dim() == 3 and hw.shape[2] == 2, tuple(hw.shape)
        n, t = int(hw.shape[0]), int(hw.shape[1])
        offset = batch["raw_offset"] if "raw_offset" in batch else raw_offsets(hw, self._resize.channels)
        frames = torch.empty(n, t, size, size, self._resize.channels, dtype=torch.uint8, device=self.device)
        self._resize(batch[key + "_raw"], offset, hw, out=frames)
        rest = {k: v for k, v in batch.items() if k not in (key + "_raw", "raw_hw", "raw_offset")}
        rest[key + "_u8"] = frames
        return rest

    def _u8_stem(self) -> bool:
        return bool(self.cfg.MODEL.get("U8_STEM", False))

    # ---- MODEL.POOL_STEM: on the pooled routes (ResidentTrainSet batches, pooled run_eval) the batch carries, under the float
    #      key, the PoolClips FramePool.clip made for stem_channels(): the stems read the arena through its index table
    def _pool_stem(self) -> bool:
        return bool(self.cfg.MODEL.get("POOL_STEM", False))

    def stem_channels(self) -> list:
        """the (c0, c) range of the 21 loader channels each pathway's stem reads: BGR+UV, or BGR+UV and the 15 flow channels"""
        if self.arch == "canonical8x8":
            raise ValueError("MODEL.POOL_STEM: the canonical8x8 stems read the float clip's three BGR planes through their "
                             "production kernels, which have no uint8 source")
        return [(0, 5), (5, 15)] if "slowfast" in self.cfg.MODEL.NAME else [(0, 5)]

    def _pool_clips(self, batch):
        """the batch's PoolClips (None: not such a batch), refusing a 'jitter' entry as _u8_clips does"""
        x = batch.get(self.cfg.MODEL.R3D_INPUT)
        if not is_pool_clips(x):
            return None
        if "jitter" in batch:
            raise ValueError(self._NO_FLOAT_CLIP.format("POOL_STEM"))
        if "mix" in batch:
            raise ValueError(self._NO_FLOAT_CLIP_MIX.format("POOL_STEM"))
        if "warp" in batch:
            raise ValueError(self._NO_FLOAT_CLIP_WARP.format("POOL_STEM"))
        return list(x)

    _NO_FLOAT_CLIP = ("MODEL.{0}: true reads the uint8 frames in the stems, so there is no float clip for the "
                      "batch's 'jitter' entry to work on; turn {0} or MODEL.COLOR_JITTER off")
    _NO_FLOAT_CLIP_WARP = ("MODEL.{0}: true reads the uint8 frames in the stems, so there is no float clip for the "
                           "batch's 'warp' entry to be sampled into; turn {0} or MODEL.AFFINE off")
    _NO_FLOAT_CLIP_MIX = ("MODEL.{0}: true reads the uint8 frames in the stems, so there is no float clip for the "
                          "batch's 'mix' entry to work on; turn {0} or MODEL.MIXUP_ALPHA / MODEL.CUTMIX_ALPHA off")

    def _u8_float(self, batch) -> torch.Tensor:
        """DevicePreprocess: (N,T,S,S,P) uint8 -> (N,T,P,S,S) float32 on the device, RandomCrop-ped by the batch's 'crop' or
        sampled through its 'warp' rows (MODEL.AFFINE) (then the batch's 'jitter' and 'mix', if any)"""
        if self._pre is None:
            from .input_pipeline import DevicePreprocess
            self._pre = DevicePreprocess(self.device, self.backend)
        x = self._pre(batch[self._u8_key(batch)], batch.get("crop"), warp=batch.get("warp"))
        return self._mix_clip(self._jitter_v1(x, batch), batch)

    # ---- the device-side ColorJitter: a batch carrying 'jitter' (N,8), the draws of input_pipeline.draw_color_jitter
    def color_jitter(self) -> "ColorJitter":
        if self._jit is None:
            from .input_pipeline import ColorJitter
            self._jit = ColorJitter(self.device, self.backend)
        return self._jit

    # ---- the device-side Mixup / CutMix: a batch carrying 'mix', the (N,8) device table of input_pipeline.ClipMix.load
    def clip_mix(self, batch_size: int = 1) -> "ClipMix":
        """the ClipMix object, its table grown to batch_size rows (the Trainer asks once, before the first step)"""
        if self._mix is None or self._mix.table.shape[0] < batch_size:
            from .input_pipeline import ClipMix
            self._mix = ClipMix(self.device, self.backend, batch_size)
        return self._mix

    def _mix_clip(self, x: torch.Tensor, batch) -> torch.Tensor:
        """Mixup / CutMix of the float (N,T,C,S,S) clip with its partner clip, in place, when the batch carries 'mix': after
        the crop and the jitter, before the permute and the channel slices, so one launch serves both pathways.  The
        channels the model reads are mixed (mix_channels), the others stay as they are."""
        if "mix" not in batch:
            return x
        return self.clip_mix()(x, batch["mix"], 0, min(self.mix_channels(), x.shape[2]))

    def mix_channels(self) -> int:
        """the leading channels of the (N,T,21,S,S) loader clip the model reads, which are the ones worth mixing: B, G, R for the
        canonical stems, BGR+UV and the flow (the depth channel, 20, is dropped) for SlowFast, BGR+UV for res3d and res2d"""
        if self.arch == "canonical8x8":
            return 3
        return 20 if "slowfast" in self.cfg.MODEL.NAME else 5

    @staticmethod
    def _own(x: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
        """x as a unit-stride tensor that is not the loader's own memory (the jitter and the mix work in place)"""
        if x.stride(-1) != 1:
            return x.contiguous()
        return x.clone() if x.untyped_storage().data_ptr() == src.untyped_storage().data_ptr() else x

    def _float_clip(self, batch) -> torch.Tensor:
        """the float32 (N,T,21,S,S) loader batch on the device (then the batch's 'jitter' and 'mix', if any)"""
        src = batch[self.cfg.MODEL.R3D_INPUT]
        if "warp" in batch:
            raise ValueError("a 'warp' entry beside a float32 loader batch: the loader has already cropped the clip, the affine "
                             "sampling (MODEL.AFFINE) needs the uint8 transport or MODEL.RESIDENT_TRAIN")
        x = self._h2d(src)
        if "jitter" not in batch and "mix" not in batch:
            return x
        return self._mix_clip(self._jitter_v1(self._own(x, src), batch), batch)

    def _jitter_v1(self, x: torch.Tensor, batch) -> torch.Tensor:
        """ColorJitter on channels 0..2 (B, G, R: cv2.imread order) of the normalised (N,T,21,S,S) clip, in place, when the
        batch carries 'jitter'.  It runs where the reference's commented-out call sits (dataset/chalearn_dataset.py:87, after
        the RandomCrop), but on IMAGE values: each stored value is de-normalised (s*0.225 + 0.45), jittered and normalised
        again.  The crop's padding is stored 0, that is image value 0.45, and is jittered like any other pixel."""
        if "jitter" not in batch:
            return x
        from .input_pipeline import MEAN, STD
        return self.color_jitter()(x, batch["jitter"], 0, True, MEAN, STD)

    def _u8_clips(self, batch, channels) -> list:
        """U8Clips over the pinned-H2D frames and crop, one per (c0, c) channel range"""
        from .input_pipeline import normalize_lut, u8_pathways
        if "jitter" in batch:
            raise ValueError(self._NO_FLOAT_CLIP.format("U8_STEM"))
        if "mix" in batch:
            raise ValueError(self._NO_FLOAT_CLIP_MIX.format("U8_STEM"))
        if "warp" in batch:
            raise ValueError(self._NO_FLOAT_CLIP_WARP.format("U8_STEM"))
        if self._lut is None:
            self._lut = normalize_lut().to(self.device)
        frames = self._h2d(batch[self._u8_key(batch)])
        assert frames.dtype == torch.uint8 and frames.dim() == 5
        if frames.stride(4) != 1:
            frames = frames.contiguous()
        crop = batch.get("crop")
        if crop is not None:
            crop = self._h2d(crop.to(torch.int32)).contiguous()
        return u8_pathways(frames, crop, self._lut, channels)

    # ---- res2d (train.py:64-76): host plumbing (res2d.py), or the engine with MODEL.RES2D_BACKEND = 'engine'
    def _res2d_backend(self) -> str:
        b = str(self.cfg.MODEL.get("RES2D_BACKEND", "torch")).lower()
        if b not in ("torch", "engine"):
            raise ValueError(f"MODEL.RES2D_BACKEND={b!r}: 'torch' or 'engine'")
        return b

    def _init_res2d_model(self):
        if self._res2d_backend() == "engine":
            from .slowfast import _DTYPES, resnet50_2d_engine
            dtype = _DTYPES[str(self.cfg.MODEL.get("DTYPE", "fp32")).lower()]
            return resnet50_2d_engine(1000, int(self.cfg.CHALEARN.CLIP_LEN), crop_resize_dict[self.cfg.MODEL.R3D_INPUT],
                                      dtype=dtype, device=self.device, backend=self.backend)
        from .res2d import resnet50_2d
        return resnet50_2d(in_channels=5 * int(self.cfg.CHALEARN.CLIP_LEN), num_classes=1000).to(
            "cpu" if torch.device(self.device).type != "cuda" else self.device)

    def _prepare_res2d_data(self, batch):
        """(N,T,21,S,S)[:, :, :5] -> (N, T*5, S, S): frames stacked on the channel axis (train.py:70-76).  Engine backend:
        the pinned (N,T,21,S,S) batch on the device, handed over as the strided (N,T,5,S,S) view -- no reshape copy; the
        stem reads frame t, channel c as input channel t*5 + c (Engine.input_view)."""
        batch = self._resized(batch)
        if self._res2d_backend() == "engine":
            clips = self._pool_clips(batch)              # MODEL.POOL_STEM on a pooled route
            if clips is not None:
                return clips[0], self._h2d(batch['label'])
            if self._u8_key(batch):                      # the uint8 transport
                if self._u8_stem():
                    return self._u8_clips(batch, [(0, 5)])[0], self._h2d(batch['label'])
                return self._u8_float(batch)[:, :, :5], self._h2d(batch['label'])
            return self._float_clip(batch)[:, :, :5], self._h2d(batch['label'])
        if "jitter" in batch:
            raise ValueError("a 'jitter' entry needs MODEL.RES2D_BACKEND = 'engine' (the torch backend has no device kernels)")
        if "mix" in batch:
            raise ValueError("a 'mix' entry needs MODEL.RES2D_BACKEND = 'engine' (the torch backend has no device kernels)")
        if "warp" in batch:
            raise ValueError("a 'warp' entry needs MODEL.RES2D_BACKEND = 'engine' (the torch backend has no device kernels)")
        dev = "cpu" if torch.device(self.device).type != "cuda" else self.device
        x = batch[self.cfg.MODEL.R3D_INPUT][:, :, :5].to(dev)
        n, t, c, h, w = x.size()
        return torch.reshape(x, (n, t * c, h, w)), batch['label'].to(dev)

    # ---- canonical SlowFast-R50 8x8 (MODEL.ARCH)
    def _init_canonical_model(self):
        from .slowfast import init_canonical_slowfast
        model = init_canonical_slowfast(self.cfg, device=self.device, backend=self.backend)
        ckpt = Path('pretrained', 'SLOWFAST_8x8_R50.pyth')          # the hub checkpoint loads as it is (no surgery)
        if ckpt.is_file():
            state = torch.load(ckpt, map_location="cpu", weights_only=True)["model_state"]
            if tuple(state['blocks.6.proj.weight'].shape) != (self.cfg.CHALEARN.NUM_CLASS, 2304):
                del state['blocks.6.proj.weight'], state['blocks.6.proj.bias']
            self.load_pretrained(model, state)
        return model

    def _prepare_canonical_data(self, batch):
        """(N,T,21,S,S) -> the BGR frames as one strided (N,3,T,S,S) view, handed over as BOTH pathways: the slow
        pathway's PackPathway gather (model.slow_t_index) happens inside its stem kernel."""
        x = torch.permute(self._float_clip(batch), [0, 2, 1, 3, 4])[:, 0:3]
        return [x, x], self._h2d(batch['label'])

    fresh_keys = None          # the model keys the pretrained load left untouched (load_pretrained); None: nothing was loaded

    def load_pretrained(self, model, state):
        """load_state_dict(state, strict=False), and record which keys it left untouched: the selectors '@fresh' and
        '@pretrained' of Engine.param_segments resolve against them.  Without a checkpoint file nothing is loaded and every
        key is fresh."""
        res = model.load_state_dict(state, strict=False)
        self.fresh_keys = set(res.missing_keys)
        eng = getattr(model, "engine", None)
        if eng is not None:
            eng.fresh_keys = set(self.fresh_keys)
        return res

    @staticmethod
    def delete_mismatch(state_dict):
        """The 12 Kinetics-checkpoint tensors whose shapes differ from the ChaLearn model (train.py:93-111)."""
        keys = ['blocks.0.multipathway_blocks.0.conv.weight', 'blocks.0.multipathway_blocks.1.conv.weight',
                'blocks.6.proj.weight', 'blocks.6.proj.bias']
        for b in (1, 2, 3, 4):
            keys += [f'blocks.{b}.multipathway_blocks.0.res_blocks.0.branch1_conv.weight',
                     f'blocks.{b}.multipathway_blocks.0.res_blocks.0.branch2.conv_a.weight']
        for k in keys:
            del state_dict[k]
        return state_dict

    def _init_slowfast_model(self):
        model = init_my_slowfast(self.cfg, (5, 15), (64, 8), device=self.device, backend=self.backend)
        ckpt = Path('pretrained', 'SLOWFAST_8x8_R50.pyth')          # train.py:116 (absent offline: random init)
        if ckpt.is_file():
            state = torch.load(ckpt, map_location="cpu", weights_only=True)["model_state"]
            self.load_pretrained(model, self.delete_mismatch(state))
        else:
            print(f'warning: {ckpt} not found, training from the reference init scheme')
        return model

    def _init_res3d_model(self):
        """slow_r50 (400 Kinetics classes, as the hub model the reference loads) with Conv3d(5, 64, (1,7,7)) as stem;
        no pretrained file exists offline, so the reference init scheme is used."""
        from .slowfast import _DTYPES, slow_r50
        dtype = _DTYPES[str(self.cfg.MODEL.get("DTYPE", "fp32")).lower()]
        t = int(self.cfg.CHALEARN.CLIP_LEN)
        s = crop_resize_dict[self.cfg.MODEL.R3D_INPUT] // 32
        # hub head pool (8,7,7) fits 8x224^2 clips; other geometries pool the whole res5 map they produce
        pool = (8, 7, 7) if (t >= 8 and s >= 7) else (min(t, 8), s, s)
        return slow_r50(400, 5, dtype=dtype, device=self.device, backend=self.backend, head_pool_kernel=pool)

    def _prepare_res3d_data(self, batch):
        """(N,T,21,S,S) -> BGR+UV (N,5,T,S,S) strided view (train.py:85-89; 5 channels as train.py:72 / the 5-channel
        stem of :81).  A uint8 batch: DevicePreprocess's float clip, or (MODEL.U8_STEM) a U8Clip over channels 0:5."""
        batch = self._resized(batch)
        clips = self._pool_clips(batch)                  # MODEL.POOL_STEM on a pooled route
        if clips is not None:
            return clips[0], self._h2d(batch['label'])
        if self._u8_key(batch):
            if self._u8_stem():
                return self._u8_clips(batch, [(0, 5)])[0], self._h2d(batch['label'])
            x = self._u8_float(batch)
        else:
            x = self._float_clip(batch)
        x = torch.permute(x, [0, 2, 1, 3, 4])
        return x[:, 0:5], self._h2d(batch['label'])

    def _prepare_slowfast_data(self, batch):
        """(N,T,21,S,S) -> [BGR+UV (N,5,T,S,S), flow (N,15,T,S,S)] strided views of the SAME memory; the depth channel
        (20) is dropped (train.py:125-145).  The stem kernels read these views in place.
        A batch that carries ``<R3D_INPUT>_u8`` (N,T,S,S,21 uint8 frames, optional ``crop`` (N,2)) instead of the float32
        tensor takes the uint8 transport: normalise + RandomCrop run on the device (input_pipeline.py), or, with
        MODEL.U8_STEM, inside the two stems, which read the frames as U8Clips over channels 0:5 and 5:20.
        An optional ``jitter`` (N,8) entry applies ColorJitter to the B, G, R planes of the float clip (_jitter_v1); an
        optional ``mix`` entry (the device table of ClipMix.load) then mixes the clip with its partner (_mix_clip)."""
        batch = self._resized(batch)
        clips = self._pool_clips(batch)                  # MODEL.POOL_STEM on a pooled route: PoolClips over channels 0:5 and 5:20
        if clips is not None:
            return clips, self._h2d(batch['label'])
        if self._u8_key(batch):
            if self._u8_stem():
                return self._u8_clips(batch, [(0, 5), (5, 15)]), self._h2d(batch['label'])
            x = self._u8_float(batch)
        else:
            x = self._float_clip(batch)
        x = torch.permute(x, [0, 2, 1, 3, 4])
        y_true = self._h2d(batch['label'])
        return [x[:, 0:5], x[:, 5:20]], y_true


def _identity(x):
    return x


class SyntheticChalearn(torch.utils.data.Dataset):
    """Stand-in with the item contract of the reference's ChalearnVideoDataset (dataset/chalearn_dataset.py:162-185):
    train -> dict, test -> list of dicts (uniform windows), values normalised like ToTensor+Normalize(0.45, 0.225).
    pooled=True: a test / valid item is ONE pooled video (input_pipeline.make_pooled_item) of F random frames, F drawn per
    video from frames_per_video = (lo, hi), with the windows of ``uniform_windows(F, CLIP_LEN)``; nclips[i] is their count.
    raw=True: the raw transport's items (input_pipeline.make_raw_item / make_raw_pooled_item) -- every frame a crop of ragged
    (h, w), each side drawn from raw_side = (lo, hi) by a generator of the frame's own; a train item keeps the uint8 item's
    'crop' (and 'jitter'), a test / valid item is one raw pooled video (raw implies pooled there).
    Under MODEL.AFFINE a uint8 or raw train item carries 'warp' (6,) float32 (input_pipeline.draw_affine) instead of 'crop'.
    An as_uint8 or raw set also offers what ``input_pipeline.ResidentTrainSet`` reads a train set through: ``seq_len(i)``
    (vframes[i], drawn per video from frames_per_video by a generator of its own), ``label(i)`` and ``video_item(i, indices)``,
    whose frame k of video i has the same bytes however it is asked for.  The items above keep their bytes."""

    def __init__(self, cfg, name_of_set: str, num_videos: int = 8, clips_per_video=(1, 3), seed: int = 0,
                 as_uint8: bool = False, pooled: bool = False, frames_per_video=(8, 40), raw: bool = False,
                 raw_side=(24, 96)):
        self.cfg, self.name = cfg, name_of_set
        self.as_uint8 = as_uint8          # hand over the HWC uint8 frames (+ the train clip's crop offsets) instead
        self.key = cfg.MODEL.R3D_INPUT
        self.size = crop_resize_dict[self.key]
        self.t = cfg.CHALEARN.CLIP_LEN
        g = torch.Generator().manual_seed(seed)
        self.labels = torch.randint(0, cfg.CHALEARN.NUM_CLASS, (num_videos,), generator=g).tolist()
        self.nclips = torch.randint(clips_per_video[0], clips_per_video[1] + 1, (num_videos,), generator=g).tolist()
        self.seed = seed
        self.raw, self.raw_side = bool(raw), (int(raw_side[0]), int(raw_side[1]))
        if self.raw:                      # only a raw set has one (Trainer._make_loaders)
            from .input_pipeline import collate_raw
            self.collate_fn = collate_raw
        self.pooled = (bool(pooled) or self.raw) and name_of_set != 'train'
        if self.pooled:                   # a generator of its own: the draws above are what they are without the flag
            from .input_pipeline import uniform_windows
            gp = torch.Generator().manual_seed(seed * 104729 + 1)
            lo, hi = frames_per_video
            self.nframes = torch.randint(int(lo), int(hi) + 1, (num_videos,), generator=gp).tolist()
            self.windows = [uniform_windows(f, self.t) for f in self.nframes]
            self.nclips = [int(w.shape[0]) for w in self.windows]
        gv = torch.Generator().manual_seed(seed * 86028121 + 3)                 # the resident view's frame counts: its own draws
        self.vframes = torch.randint(int(frames_per_video[0]), int(frames_per_video[1]) + 1, (num_videos,), generator=gv).tolist()

    def __len__(self):
        return len(self.labels)

    # ---- what input_pipeline.ResidentTrainSet reads a train set through
    def seq_len(self, i) -> int:
        return self.vframes[i]

    def label(self, i) -> int:
        return self.labels[i]

    def _video_frame(self, i, k):
        """frame k of video i of the resident view: (S, S, 21) random bytes, or ragged ones (raw), a generator of its own"""
        g = torch.Generator().manual_seed((self.seed * 32452843 + i) * 4099 + k)
        if self.raw:
            h, w = torch.randint(self.raw_side[0], self.raw_side[1] + 1, (2,), generator=g).tolist()
            return torch.randint(0, 256, (h, w, 21), generator=g, dtype=torch.uint8)
        return torch.randint(0, 256, (self.size, self.size, 21), generator=g, dtype=torch.uint8)

    def video_item(self, i, indices=None) -> dict:
        from .input_pipeline import make_pooled_item, make_raw_pooled_item
        if not (self.as_uint8 or self.raw):
            raise ValueError("SyntheticChalearn.video_item: a float32 set has no uint8 frames; build it with as_uint8=True or raw=True")
        indices = list(range(self.vframes[i])) if indices is None else [int(k) for k in indices]
        assert all(0 <= k < self.vframes[i] for k in indices), (i, indices)
        make = make_raw_pooled_item if self.raw else make_pooled_item
        return make(self.key, [indices], self.labels[i], lambda k: self._video_frame(i, k))

    def _raw_frame(self, i, j, k):
        """frame k of clip j (or of the pooled video, j = -1) of video i: ragged (h, w, 21) random bytes, a generator of its own"""
        g = torch.Generator().manual_seed(((self.seed * 15485863 + i) * 1009 + j + 1) * 2003 + k)
        lo, hi = self.raw_side
        h, w = torch.randint(lo, hi + 1, (2,), generator=g).tolist()
        return torch.randint(0, 256, (h, w, 21), generator=g, dtype=torch.uint8)

    def _pooled(self, i):
        from .input_pipeline import make_pooled_item
        if self.raw:
            from .input_pipeline import make_raw_pooled_item
            return make_raw_pooled_item(self.key, self.windows[i], self.labels[i], lambda k: self._raw_frame(i, -1, k))
        g = torch.Generator().manual_seed(self.seed * 7919 + i * 31 + 17)
        frames = torch.randint(0, 256, (self.nframes[i], self.size, self.size, 21), generator=g, dtype=torch.uint8)
        return make_pooled_item(self.key, self.windows[i], self.labels[i], lambda k: frames[k])

    def _clip(self, i, j):
        g = torch.Generator().manual_seed(self.seed * 7919 + i * 31 + j)
        u8 = torch.randint(0, 256, (self.t, 21, self.size, self.size), generator=g, dtype=torch.uint8)
        if self.raw:                      # (u8 is drawn all the same: 'crop' and 'jitter' below are the uint8 item's draws)
            from .input_pipeline import make_raw_item
            item = make_raw_item(self.key, [self._raw_frame(i, j, k) for k in range(self.t)], self.labels[i])
            if self.name == 'train':                 # 'crop', or 'warp' under MODEL.AFFINE
                k, row = draw_crop_or_warp(self.cfg, self.size, g)
                item[k] = row
        elif self.as_uint8:
            item = {self.key + "_u8": u8.permute(0, 2, 3, 1).contiguous(), 'label': self.labels[i]}
            if self.name == 'train':                 # 'crop', or 'warp' under MODEL.AFFINE
                k, row = draw_crop_or_warp(self.cfg, self.size, g)
                item[k] = row
        else:
            item = {self.key: (u8.float() / 255.0 - 0.45) / 0.225, 'label': self.labels[i]}
        ranges = jitter_ranges(self.cfg) if self.name == 'train' else None
        if ranges is not None:                       # MODEL.COLOR_JITTER: the train clip's ColorJitter draws
            from .input_pipeline import draw_color_jitter
            item['jitter'] = draw_color_jitter(1, *ranges, generator=g)[0]
        return item

    def __getitem__(self, i):
        if self.name == 'train':
            return self._clip(i, 0)
        if self.pooled:
            return self._pooled(i)
        return [self._clip(i, j) for j in range(self.nclips[i])]


def cv2_read_frame(path, size: int):
    """One frame's (size, size, 21) uint8 HWC image as the reference builds it (dataset/chalearn_dataset.py:99-116): the BGR
    image, its U_ and V_ gray images, the five 3-channel flow images F0_ .. F4_ and the D_ gray image beside it, concatenated
    on the channel axis, zero-padded to a square about its centre and resized with cv2.INTER_CUBIC; None when the file is
    missing.  cv2 is imported here, on first use."""
    try:
        import cv2
    except Exception as e:
        raise RuntimeError("ChalearnVideoFramesU8's default frame reader needs OpenCV (cv2), which is not importable here "
                           f"({e}); install it or pass read_frame=") from e
    path = Path(path)
    if not path.exists():
        return None

    def side(prefix, gray):
        f = str(Path(path.parent, prefix + path.name))
        return cv2.imread(f, cv2.IMREAD_GRAYSCALE)[..., np.newaxis] if gray else cv2.imread(f)

    img = np.concatenate([cv2.imread(str(path)), side('U_', True), side('V_', True)] +
                         [side(f'F{k}_', False) for k in range(5)] + [side('D_', True)], axis=-1)
    h, w, c = img.shape
    m = max(h, w)
    nx, ny = (m - w) // 2, (m - h) // 2
    sq = np.zeros((m, m, c), dtype=img.dtype)
    sq[ny:ny + h, nx:nx + w, :] = img
    return cv2.resize(sq, (size, size), interpolation=cv2.INTER_CUBIC)


def cv2_read_frame_raw(path):
    """``cv2_read_frame`` without the pad and the resize: the (h, w, 21) uint8 HWC concatenation of a frame's images at the
    crop's own size (dataset/chalearn_dataset.py:99-113), for the raw transport -- ``PadResize`` does the rest on the
    device; None when the file is missing."""
    try:
        import cv2
    except Exception as e:
        raise RuntimeError("ChalearnVideoFramesU8's default raw frame reader needs OpenCV (cv2), which is not importable "
                           f"here ({e}); install it or pass read_frame=") from e
    path = Path(path)
    if not path.exists():
        return None

    def side(prefix, gray):
        f = str(Path(path.parent, prefix + path.name))
        return cv2.imread(f, cv2.IMREAD_GRAYSCALE)[..., np.newaxis] if gray else cv2.imread(f)

    return np.concatenate([cv2.imread(str(path)), side('U_', True), side('V_', True)] +
                          [side(f'F{k}_', False) for k in range(5)] + [side('D_', True)], axis=-1)


class ChalearnVideoFramesU8(torch.utils.data.Dataset):
    """The reference's ChalearnVideoDataset (dataset/chalearn_dataset.py:26-185) for the uint8 transport: normalisation and
    the RandomCrop are left to the device, and a test video is handed over as ONE pooled item instead of its windows.

    labels: the reference's ``get_labels(name_of_set)`` list of (rgb path, depth path, 1-based label) (default: that call,
    when the reference's utils.chalearn is importable).  'train': one ``random_sampling`` window,
    {'<R3D_INPUT>_u8': (T, S, S, 21) uint8, 'crop': (2,) int32, 'label': label - 1} (+ 'jitter' under MODEL.COLOR_JITTER;
    under MODEL.AFFINE 'warp': (6,) float32, the row of input_pipeline.draw_affine, takes the place of 'crop', here and below).
    'test' / 'valid': {'<R3D_INPUT>_pool': (F, S, S, 21) uint8, 'windows': (K, T) int32, 'label'} -- the frames some uniform
    window references, each read ONCE, a missing frame file as -1 -- or, with pooled=False, the list of
    {'<R3D_INPUT>_u8', 'label'} clips.  read_frame(path, size) -> (size, size, 21) uint8 or None is injectable (default:
    ``cv2_read_frame``).
    resize='device': the raw transport.  read_frame(path) -> (h, w, 21) uint8 at the crop's own size, or None (default:
    ``cv2_read_frame_raw``); 'train': {'<R3D_INPUT>_raw': 1-D uint8, 'raw_hw': (T, 2) int32, 'crop', 'label'} (+ 'jitter'),
    a missing frame as (0, 0); 'test' / 'valid': {'<R3D_INPUT>_rawpool': 1-D uint8, 'raw_hw': (F, 2) int32, 'windows',
    'label'}.  The set then has ``collate_fn = collate_raw``, which the Trainer's train loader uses.
    ``seq_len(i)`` (the number of frame names, no image read), ``label(i)`` and ``video_item(i, indices=None)`` (one pooled
    item, or raw pooled item, over those frames of the video, default all) are what ``input_pipeline.ResidentTrainSet`` reads
    a train set through (MODEL.RESIDENT_TRAIN)."""

    def __init__(self, cfg, name_of_set: str, labels=None, read_frame: Optional[Callable] = None, pooled: bool = True,
                 resize: str = "host"):
        assert name_of_set in ("train", "test", "valid")
        if resize not in ("host", "device"):
            raise ValueError(f"resize={resize!r}: 'host' or 'device'")
        if resize == "device" and name_of_set != "train" and not pooled:
            raise ValueError("resize='device' hands a test video over as one raw pooled item: pooled=False has no raw form")
        self.resize = resize
        if resize == "device":
            from .input_pipeline import collate_raw
            self.collate_fn = collate_raw
        if labels is None:
            try:
                from utils.chalearn import get_labels               # the reference's module, unchanged
            except Exception as e:
                raise RuntimeError(f"no labels were given and the reference's utils.chalearn is not importable here ({e})") from e
            labels = get_labels(name_of_set)
        self.cfg, self.name, self.labels = cfg, name_of_set, list(labels)
        self.key = cfg.MODEL.R3D_INPUT
        self.size = crop_resize_dict[self.key]
        self.clip_len = int(cfg.CHALEARN.CLIP_LEN)
        self.read_frame = read_frame or (cv2_read_frame_raw if resize == "device" else cv2_read_frame)
        self.pooled = bool(pooled)
        import random
        self.rng = random

    def __len__(self):
        return len(self.labels)

    def _video(self, index):
        """(the video's folder below a crop folder, its sorted frame file names, label - 1): :163-169"""
        m, _k, l = self.labels[index]
        folder = Path(m).parent / Path(m).stem
        files = sorted(glob.glob(str(Path(self.cfg.CHALEARN.ROOT, self.cfg.CHALEARN.IMG, folder) / "*")))
        return folder, [Path(f).name for f in files], int(l) - 1

    def seq_len(self, index) -> int:
        return len(self._video(index)[1])                # the reference's len(img_names), :163-169

    def label(self, index) -> int:
        return int(self.labels[index][2]) - 1

    def video_item(self, index, indices=None) -> dict:
        from .input_pipeline import make_pooled_item, make_raw_pooled_item
        folder, names, label = self._video(index)
        indices = list(range(len(names))) if indices is None else [int(k) for k in indices]
        if self.resize == "device":
            return make_raw_pooled_item(self.key, [indices], label, lambda i: self._read_raw(folder, names[i]))
        return make_pooled_item(self.key, [indices], label, lambda i: self._read(folder, names[i]))

    def _read(self, folder, name):
        f = self.read_frame(Path(self.cfg.CHALEARN.ROOT, self.key, folder, name), self.size)
        if f is None:
            return None
        f = torch.as_tensor(f)
        assert f.dtype == torch.uint8 and tuple(f.shape) == (self.size, self.size, 21), (f.dtype, tuple(f.shape))
        return f

    def _read_raw(self, folder, name):
        f = self.read_frame(Path(self.cfg.CHALEARN.ROOT, self.key, folder, name))
        if f is None:
            return None
        f = torch.as_tensor(f)
        assert f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 21, (f.dtype, tuple(f.shape))
        return f

    def __getitem__(self, index):
        from .input_pipeline import (MISSING_BYTE, draw_color_jitter, make_pooled_item, make_raw_item, make_raw_pooled_item,
                                     uniform_windows, unpool_item)
        folder, names, label = self._video(index)
        seq_len = len(names)
        if self.name == "train":
            start = self.rng.randint(0, max(0, seq_len - self.clip_len))           # random_sampling, :123-129
            if self.resize == "device":
                item = make_raw_item(self.key, [self._read_raw(folder, names[i % seq_len])
                                                for i in range(start, start + self.clip_len)], label)
                k, row = draw_crop_or_warp(self.cfg, self.size)     # 'crop', or 'warp' under MODEL.AFFINE
                item[k] = row
                ranges = jitter_ranges(self.cfg)
                if ranges is not None:
                    item["jitter"] = draw_color_jitter(1, *ranges)[0]
                return item
            frames = []
            for i in range(start, start + self.clip_len):
                f = self._read(folder, names[i % seq_len])
                frames.append(torch.full((self.size, self.size, 21), MISSING_BYTE, dtype=torch.uint8) if f is None else f)
            k, row = draw_crop_or_warp(self.cfg, self.size)
            item = {self.key + "_u8": torch.stack(frames), k: row, "label": label}
            ranges = jitter_ranges(self.cfg)
            if ranges is not None:
                item["jitter"] = draw_color_jitter(1, *ranges)[0]
            return item
        if self.resize == "device":
            return make_raw_pooled_item(self.key, uniform_windows(seq_len, self.clip_len), label,
                                        lambda i: self._read_raw(folder, names[i]))
        item = make_pooled_item(self.key, uniform_windows(seq_len, self.clip_len), label,
                                lambda i: self._read(folder, names[i]))
        return item if self.pooled else unpool_item(item)


class Trainer:
    def __init__(self, cfg, train_loader=None, test_loader=None, device="cuda", backend=None, use_graph: bool = False,
                 train_set=None, test_set=None, dist_backend: Optional[str] = None):
        """train_set / test_set: datasets with the reference's item contract (default: the reference's own
        ChalearnVideoDataset); the Trainer builds the loaders from them as train.py:149-170 does and, when WORLD_SIZE > 1,
        shards them over the ranks.  train_loader / test_loader: ready loaders, used as they are."""
        self.debug = cfg.DEBUG
        self.num_workers = 0 if self.debug else min(cfg.NUM_CPU, 10)
        self.cfg = cfg
        self.device = device
        self.batch_size = cfg.CHALEARN.BATCH_SIZE
        self.rank, self.world, _ = sdist.init_process_group_from_env(dist_backend)
        self.epoch = 0
        if train_loader is None or test_loader is None:
            if train_set is None or test_set is None:
                train_set, test_set = self._reference_datasets()
            train_loader, test_loader = self._make_loaders(train_set, test_set)
        self.train_loader, self.test_loader = train_loader, test_loader
        self.mm = self._model_manager(cfg, device, backend)
        self.pool_stem = self._check_pool_stem()
        if bool(cfg.MODEL.get("RESIDENT_TRAIN", False)):
            self.resident = self._make_resident(train_set, backend)
        self.model = self.mm.init_model()
        self.num_step = 0
        self.ckpt_dir = Path(cfg.CHALEARN.ROOT, cfg.MODEL.LOGS, cfg.MODEL.CKPT_DIR, cfg.MODEL.NAME)
        self.max_historical_acc = 0.
        self.load_ckpt()
        eng = getattr(self.model, "engine", None)
        self.label_smoothing, self.mix_draw, self.mix_seed = mix_settings(cfg)
        self.ema_decay, self.ema_warmup, self.ema_eval = ema_settings(cfg)
        # Adam is created AFTER the checkpoint load, its state is never saved (train.py:180-182)
        if eng is None:                                  # res2d: a plain torch module, the reference's own five lines
            from .res2d import TorchStep
            assert self.world == 1, "res2d is single-process host plumbing"
            if self._optim_kwargs():
                raise ValueError("MODEL.LR_SCHEDULE / WEIGHT_DECAY / CLIP_GRAD_NORM need the engine's optimizer launch: MODEL.NAME "
                                 "res2d with the torch backend is host plumbing (torch.optim.Adam); use RES2D_BACKEND = 'engine'")
            if self.label_smoothing > 0 or self.mix_draw is not None:
                raise ValueError("MODEL.LABEL_SMOOTHING / MIXUP_ALPHA / CUTMIX_ALPHA need the engine's loss launch: MODEL.NAME res2d "
                                 "with the torch backend is host plumbing (nn.CrossEntropyLoss); use RES2D_BACKEND = 'engine'")
            if self.ema_decay > 0:
                raise ValueError("MODEL.EMA_DECAY needs the engine's parameter arena and its sfk_ema_update launch: MODEL.NAME res2d "
                                 "with the torch backend is host plumbing (torch.optim.Adam); use RES2D_BACKEND = 'engine'")
            if self._group_kwargs():
                raise ValueError("MODEL.PARAM_GROUPS / FREEZE need the engine's parameter arena and its sfk_adam_groups launch: "
                                 "MODEL.NAME res2d with the torch backend is host plumbing (torch.optim.Adam); use RES2D_BACKEND = "
                                 "'engine'")
            self.step = TorchStep(self.model, lr=cfg.MODEL.LR)
        else:
            reducer = sdist.GradReducer(eng.G, bucket_mb=cfg.DIST.BUCKET_MB) if self.world > 1 else None
            self.step = self._make_step(eng, use_graph, reducer)
            if self.step.ema is not None:
                # the average starts from the weights load_ckpt left.  A fresh engine's average is that copy already
                # (Engine.optim_state); this matters for an engine whose average existed before this trainer
                self.step.ema.reset()
            if self.mix_draw is not None:                # the one device table every step's rows are written into
                self.mm.clip_mix(int(self.batch_size))

    # ---- what a derived trainer (gesture_v2.Trainer) swaps: the model manager, the optimiser, the train loader's drop_last
    train_drop_last = True                               # train.py:164

    def _model_manager(self, cfg, device, backend):
        return ModelManager(cfg, device=device, backend=backend)

    def steps_per_epoch(self) -> int:
        """optimizer steps of one train_epoch: the resident plan's batches, else len(train_loader)"""
        resident = getattr(self, "resident", None)
        if resident is not None:
            n, bs = len(resident.train_set), int(resident.batch_size)
            return max(n // bs if resident.drop_last else -(-n // bs), 1)
        return max(len(self.train_loader), 1)

    def _optim_kwargs(self) -> dict:
        """MODEL.LR_SCHEDULE, WEIGHT_DECAY*, CLIP_GRAD_NORM as TrainStep keywords ({} at the defaults); the table spans
        MAX_EPOCH * steps_per_epoch() steps and is indexed by the optimizer's own step count (schedule.py)"""
        from .schedule import optim_kwargs
        return optim_kwargs(self.cfg, self.steps_per_epoch)

    def _group_kwargs(self) -> dict:
        """MODEL.PARAM_GROUPS / FREEZE as TrainStep keywords ({} at the defaults).  The step is built after init_model's
        load_pretrained, so '@fresh' and '@pretrained' resolve against that load"""
        from .schedule import group_kwargs
        return group_kwargs(self.cfg)

    def _mix_kwargs(self) -> dict:
        """MODEL.LABEL_SMOOTHING as a TrainStep keyword ({} at the default)"""
        return {"label_smoothing": self.label_smoothing} if self.label_smoothing > 0 else {}

    def _ema_kwargs(self) -> dict:
        """MODEL.EMA_DECAY / EMA_WARMUP as TrainStep keywords ({} at the default)"""
        return {"ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup} if self.ema_decay > 0 else {}

    def mix_frame(self) -> int:
        """the side of the square frames the mix boxes are drawn on"""
        return int(crop_resize_dict[self.cfg.MODEL.R3D_INPUT])

    def _mix_generator(self) -> torch.Generator:
        """the epoch's generator of the mix draws, seeded by (MODEL.MIX_SEED, epoch, rank) and advanced per step"""
        return torch.Generator().manual_seed(((self.mix_seed * 1000003 + int(self.epoch)) * 1000003 + int(self.rank)) % (2 ** 63))

    def _attach_mix(self, batch, gen):
        """draw the batch's mix rows, write them into the device table, attach the table's first n rows as batch['mix']"""
        from .input_pipeline import draw_mix
        n, s = int(batch["label"].shape[0]), self.mix_frame()
        table = self.mm.clip_mix(n).load(draw_mix(n, s, s, generator=gen, **self.mix_draw), s, s)
        batch = dict(batch)
        batch["mix"] = table
        return batch, table

    def _make_step(self, eng, use_graph, reducer):
        return TrainStep(eng, lr=self.cfg.MODEL.LR, use_graph=use_graph, reducer=reducer, **self._optim_kwargs(),
                         **self._mix_kwargs(), **self._ema_kwargs(), **self._group_kwargs())

    def _reference_datasets(self):
        try:
            from dataset.chalearn_dataset import ChalearnVideoDataset   # the reference's module, unchanged
        except Exception as e:  # cv2 / torchvision / label files missing
            raise RuntimeError("no datasets / loaders were given and the reference's dataset.chalearn_dataset is not "
                               f"importable here ({e}); pass train_set/test_set (e.g. SyntheticChalearn)") from e
        return ChalearnVideoDataset(self.cfg, 'train'), ChalearnVideoDataset(self.cfg, 'test')

    # ---- MODEL.RESIDENT_TRAIN; a derived trainer (gesture_v2.Trainer) swaps the contract it asks for and the set it builds
    resident_methods_missing = ("seq_len(i), label(i) and video_item(i, indices=None) "
                                "(ChalearnVideoFramesU8 and SyntheticChalearn(as_uint8 / raw) do)")

    # ---- MODEL.POOL_STEM: the pooled routes hand the stems PoolClips instead of the gathered float clip
    pool_stem_unsupported = None                         # a derived trainer's reason why it cannot (gesture_v2.Trainer)

    def _check_pool_stem(self) -> bool:
        if not bool(self.cfg.MODEL.get("POOL_STEM", False)):
            return False
        why = self.pool_stem_unsupported
        if why is None and self.world > 1:
            why = "the resident set it feeds from has no per-rank partition yet: WORLD_SIZE must be 1"
        elif why is None and self.cfg.MODEL.NAME == "res2d" and self.mm._res2d_backend() == "torch":
            why = "MODEL.NAME res2d with the torch backend is host plumbing and has no stem kernels; use RES2D_BACKEND = 'engine'"
        if why is not None:
            raise ValueError(f"MODEL.POOL_STEM: {why}")
        self.mm.stem_channels()                          # (raises for an architecture without uint8 stems)
        return True

    def _offers_resident(self, train_set) -> bool:
        from .input_pipeline import offers_resident
        return offers_resident(train_set)

    def _build_resident(self, train_set, backend):
        from .input_pipeline import ResidentTrainSet
        return ResidentTrainSet(train_set, self.cfg, self.device, backend, batch_size=self.batch_size,
                                drop_last=self.train_drop_last, num_workers=self.num_workers, jitter=jitter_ranges(self.cfg),
                                stem_channels=self.mm.stem_channels() if self.pool_stem else None,
                                affine=affine_ranges(self.cfg))

    def _make_resident(self, train_set, backend):
        """MODEL.RESIDENT_TRAIN: the resident set (v1: ResidentTrainSet) train_epoch iterates instead of the train loader"""
        why = None
        if train_set is None:
            why = ("it needs the train SET (train_set=), whose frames it keeps on the device; a ready-made train_loader= only "
                   "hands over finished batches")
        elif not self._offers_resident(train_set):
            why = f"{type(train_set).__name__} does not offer {self.resident_methods_missing}"
        elif self.world > 1:
            why = "a per-rank partition of the resident set is not built yet: WORLD_SIZE must be 1"
        elif self.cfg.MODEL.NAME == "res2d" and self.mm._res2d_backend() == "torch":
            why = "MODEL.NAME res2d with the torch backend is host plumbing and has no device kernels; use RES2D_BACKEND = 'engine'"
        if why is not None:
            raise ValueError(f"MODEL.RESIDENT_TRAIN: {why}")
        return self._build_resident(train_set, backend)

    def _make_loaders(self, tr, te):
        """train.py:164,170: train = shuffle + drop_last, test = whole videos, identity collate.  world > 1: one shuffled
        epoch cut into disjoint per-rank shards (every rank runs the same number of steps), test videos round-robin."""
        pin = torch.device(self.device).type == "cuda"
        kw = dict(num_workers=self.num_workers, pin_memory=pin)
        tkw = dict(kw)                                   # the train loader: a dataset's own collate (the raw items' collate_raw)
        if getattr(tr, "collate_fn", None) is not None:
            tkw["collate_fn"] = tr.collate_fn
        if self.world > 1:
            self.train_sampler = sdist.EpochShardSampler(len(tr), self.rank, self.world, seed=0,
                                                         drop_last=self.train_drop_last)
            train = torch.utils.data.DataLoader(tr, batch_size=self.batch_size, sampler=self.train_sampler,
                                                drop_last=self.train_drop_last, **tkw)
            test = torch.utils.data.DataLoader(te, batch_size=self.batch_size, drop_last=False, collate_fn=_identity,
                                               sampler=sdist.VideoShardSampler(len(te), self.rank, self.world), **kw)
            test.sfk_shard = (self.rank, self.world, len(te))
        else:
            self.train_sampler = None
            train = torch.utils.data.DataLoader(tr, batch_size=self.batch_size, shuffle=True,
                                                drop_last=self.train_drop_last, **tkw)
            test = torch.utils.data.DataLoader(te, batch_size=self.batch_size, shuffle=False, drop_last=False,
                                               collate_fn=_identity, **kw)
        return train, test

    # ---- checkpoints: model weights only, 'acc%.3f_e%d.ckpt', newest by lexicographic sort, HTAH fallback
    def save_ckpt(self, epoch=0, acc=0.0):
        if self.rank != 0:
            return
        self.ckpt_dir.mkdir(parents=True, exist_ok=True)
        ckpt_path = Path(self.ckpt_dir, 'acc%.3f_e%d.ckpt' % (acc, epoch))
        if not self.debug:
            torch.save({k: v.cpu() for k, v in self.model.state_dict().items()}, ckpt_path)
            print(f"Checkpoint saved in {str(ckpt_path)}")
        else:
            print(f'Ignore checkpoint saving under debug mode. {str(ckpt_path)}')

    def load_ckpt(self):
        ckpt_list = sorted(glob.glob(str(self.ckpt_dir / '*.ckpt')))
        if len(ckpt_list) == 0:
            print('warning: no checkpoint found, try using HTAH ckeckpoint')
            ckpt_list = sorted(glob.glob(str(Path(self.ckpt_dir.parent, 'slowfast-HTAH', '*.ckpt'))))
            if len(ckpt_list) == 0:
                print('warning: no HTAH checkpoint found')
                return
        ckpt = ckpt_list[-1]
        print(f'loading checkpoint from {str(ckpt)}')
        self.model.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True), strict=True)

    def train_epoch(self):
        self.step.reset_meters()
        seen = 0
        self.model.train()
        if getattr(self, "train_sampler", None) is not None:
            self.train_sampler.set_epoch(self.epoch)     # a new permutation of the epoch, the same on every rank
        resident = getattr(self, "resident", None)       # MODEL.RESIDENT_TRAIN: clips gathered from the frames on the device
        mix_gen = self._mix_generator() if self.mix_draw is not None else None
        for batch in (self.train_loader if resident is None else resident.epoch(self.epoch)):
            kw = {}
            if mix_gen is not None:                      # MODEL.MIXUP_ALPHA / CUTMIX_ALPHA: the clip and the loss share one table
                batch, kw["mix"] = self._attach_mix(batch, mix_gen)
            x, y_true = self.mm.prepare_data(batch)
            if isinstance(x, (torch.Tensor,) + STEM_CLIPS):    # res3d / res2d: one input tensor (or uint8 clip)
                self.step(x, None, y_true, **kw)
            else:
                self.step(x[0], x[1], y_true, slow_t_index=self.model.slow_t_index, **kw)
            self.num_step += 1
            seen += int(y_true.shape[0])
            if self.debug:
                break
        # one device->host read per epoch instead of one per step
        loss_avg = float(self.step.loss_sum[0]) / max(self.step.steps, 1)
        correct = int(self.step.correct[0])
        if self.world > 1:                               # the epoch's meters over all ranks (printed by every rank)
            parts = sdist.gather_objects((loss_avg, correct, seen))
            loss_avg = sum(p[0] for p in parts) / len(parts)
            correct, seen = sum(p[1] for p in parts), sum(p[2] for p in parts)
        print(f'loss_avg: {round(loss_avg, 3)}')
        print(f'Train Accuracy: {round(correct / max(seen, 1), 3)}. ({correct} / {seen})')
        if getattr(self.step, "hp", False):              # the scheduled step: its last rate and gradient norm, read once an epoch
            gn = self.step.grad_norm
            if getattr(self.step.opt, "grouped", False):     # one rate per group: the unmatched rest, then PARAM_GROUPS' order
                rates = 'lr: [' + ', '.join(f'{r:.6g}' for r in self.step.last_lrs()) + ']'
            else:
                rates = f'lr: {self.step.last_lr():.6g}'
            print(rates + ('' if gn is None else f', grad_norm: {float(gn[0]):.4g}'))
        return loss_avg, correct / max(seen, 1)

    def _evaluates_average(self) -> bool:
        """MODEL.EMA_DECAY > 0 on the engine and EMA_EVAL 'ema' or 'both': train() evaluates and saves the averaged model"""
        return getattr(self.step, "ema", None) is not None and self.ema_eval != "live"

    def _averaged(self):
        """the context train() evaluates and saves in: when _evaluates_average() the engine holds the averaged weights and
        running statistics inside it (ema.WeightEma.applied) and the live ones again after it; otherwise nothing happens"""
        return self.step.ema.applied() if self._evaluates_average() else contextlib.nullcontext()

    def train(self):
        """With MODEL.EMA_DECAY > 0 (and EMA_EVAL not 'live') the epoch's evaluation and every checkpoint are the AVERAGED
        model's, in the ordinary flat state_dict format; 'both' evaluates the live model first and prints both accuracies.
        The average and its counter are not checkpointed separately, as the optimizer state is not."""
        max_epoch = self.cfg.MODEL.MAX_EPOCH if not self.debug else 3
        acc, epoch = 0.0, 0
        averaged = self._evaluates_average()
        for epoch in range(max_epoch):
            print(f'========== Training epoch {epoch}')
            self.num_step = 0
            self.epoch = epoch
            self.train_epoch()
            if averaged and self.ema_eval == "both":
                print('Live Accuracy: %.3f' % self.run_eval()['acc'])
            with self._averaged():
                acc = self.run_eval()['acc']
                if averaged:
                    print('EMA Accuracy: %.3f' % acc)
                if acc > self.max_historical_acc:
                    self.max_historical_acc = acc
                    self.save_ckpt(epoch, acc)
                else:
                    print("Not saved. Current best acc: %.3f" % (self.max_historical_acc))
        with self._averaged():
            self.save_ckpt(epoch, acc)

    def run_eval(self, dataset_loader=None):
        """Batched no-grad forward over uniform windows; softmax; per-video mean over its clips; argmax
        (train.py:287-370).  Returns {'ps','t','acc','sv'} as train_sparse.py:76-84 consumes it.
        The logits of every batch stay on the device; softmax, the per-video mean, argmax and the accuracy count are
        ONE ``sfk_eval_aggregate`` launch at the end, followed by one device->host copy of the result (the reference
        copies logits and labels to the host after every batch, train.py:308-309).
        A loader element that is a pooled item (a dict with '<R3D_INPUT>_pool' and 'windows', input_pipeline.py) is one
        video whose frames are uploaded once into ``self.frame_pool``; its windows join the batches as (video, row)
        references, and a batch of them is ONE ``sfk_u8_pool_gather`` launch that writes the float clip, handed to
        prepare_data under the float key (whatever MODEL.U8_STEM says) -- or, under MODEL.POOL_STEM, no launch at all: the
        batch is the ``PoolClip``s of ``FramePool.clip`` and the stems read the pool (include/sfk_u8stem_pool.h).  ``frame_pool.bytes_uploaded`` counts this call's.
        A raw pooled item ('<R3D_INPUT>_rawpool' + 'raw_hw': the frames at their native sizes) differs only in how its arena
        slots are filled: ``FramePool.add_raw`` uploads the raw bytes and ``sfk_u8_pad_resize_cubic`` writes the frames."""
        loader = self.test_loader if dataset_loader is None else dataset_loader
        logit_list, true_list, batch_collect, samples_per_video = [], [], [], []
        self.model.eval()
        key = self.cfg.MODEL.R3D_INPUT
        if getattr(self, "frame_pool", None) is not None:
            self.frame_pool.bytes_uploaded = 0

        def pool_video(b):
            if getattr(self, "frame_pool", None) is None:
                from .input_pipeline import FramePool
                self.frame_pool = FramePool(self.device, self.mm.backend)
            if key + "_rawpool" in b:                      # the frames at their native sizes: resized into the arena slots
                base = self.frame_pool.add_raw(b[key + "_rawpool"], b["raw_hw"], crop_resize_dict[key], b["windows"])
            else:
                base = self.frame_pool.add(b[key + "_pool"], b["windows"])
            video = {"base": base, "rows": self.frame_pool.rows(base, b["windows"]), "label": int(b["label"]),
                     "left": int(b["windows"].shape[0])}
            return [(video, r) for r in range(video["left"])]

        pool_stem = getattr(self, "pool_stem", False)          # MODEL.POOL_STEM: the stems read the pool, nothing is gathered
        read_out = []                                          # ... so a video's slots are free only once the forward that
                                                               # reads its last window has been enqueued (test_batch)

        def collate(items):
            if not isinstance(items[0], tuple):
                return default_collate(items)
            rows = torch.stack([v["rows"][r] for v, r in items])
            clip = self.frame_pool.clip(rows, self.mm.stem_channels()) if pool_stem else self.frame_pool.gather(rows)
            for v, _ in items:
                v["left"] -= 1
                if v["left"] == 0 and pool_stem:
                    read_out.append(v["base"])
                elif v["left"] == 0:                           # its last window is in this gather: the slots are free
                    self.frame_pool.release(v["base"])         # for uploads queued behind it on the same stream
            return {key: clip, "label": torch.tensor([v["label"] for v, _ in items])}

        def test_batch(collect):
            try:
                x, y_true = self.mm.prepare_data(collect)
                with torch.no_grad():
                    y_pred = self.model(x)
            finally:                                           # that forward is enqueued (or failed before it read anything):
                while read_out:                                # uploads queue behind it
                    self.frame_pool.release(read_out.pop(0))
            logit_list.append(y_pred.float().clone())      # the engine reuses its logits buffer
            true_list.append(y_true.clone())

        for step, batch in enumerate(loader):
            for b in batch:
                if isinstance(b, dict) and (key + "_pool" in b or key + "_rawpool" in b):   # a pooled video
                    b = pool_video(b)
                samples_per_video.append(len(b))
                batch_collect.extend(b)
            if len(batch_collect) < self.batch_size:
                continue
            while len(batch_collect) > self.batch_size:          # strict '>' as the reference (train.py:322)
                test_batch(collate(batch_collect[:self.batch_size]))
                batch_collect = batch_collect[self.batch_size:]
            if self.debug and step > 5:
                break
        if len(batch_collect) > 0:
            test_batch(collate(batch_collect))
        if logit_list:
            logits = torch.cat(logit_list, dim=0).contiguous()
            labels = torch.cat(true_list, dim=0).to(torch.int64).contiguous()
        else:
            # a rank whose shard holds no video (fewer test videos than ranks): zero rows, so that it still takes part in
            # the gather below instead of raising while the other ranks wait in all_gather_object
            # (the width is a placeholder: the res2d network scores 1000 classes, reference train.py:64-76; _gather_eval never
            # concatenates a zero-row part)
            logits = torch.zeros(0, int(self.cfg.CHALEARN.NUM_CLASS), dtype=torch.float32, device=self.device)
            labels = torch.zeros(0, dtype=torch.int64, device=self.device)
        shard = getattr(loader, "sfk_shard", None)
        # (debug mode stops after a few loader steps on every rank; the shards are then partial, nothing is gathered and each
        # rank reports the accuracy of its own videos -- harmless: only rank 0 writes checkpoints, debug writes none)
        if shard is not None and shard[1] > 1 and not self.debug:
            logits, labels, samples_per_video = self._gather_eval(logits, labels, samples_per_video, shard)
        if hasattr(self.model, "engine"):
            ps, pred, ncorrect = aggregate_scores(self.model.engine.be, logits, labels, samples_per_video, softmax=True)
        else:
            from .res2d import aggregate_scores_host
            ps, pred, ncorrect = aggregate_scores_host(logits, labels, samples_per_video)
        ps, true_arr = ps.cpu().numpy(), labels.cpu().numpy()
        nvid = sum(1 for s_ in samples_per_video if s_ > 0)
        accuracy = ncorrect / max(nvid, 1)
        print(f'Test Accuracy: {round(float(accuracy), 3)}. ({ncorrect} / {nvid})')
        return {'ps': ps, 't': true_arr, 'acc': accuracy, 'sv': samples_per_video}


    def _gather_eval(self, logits, labels, sv, shard):
        """every rank evaluated videos rank, rank + world, ... (VideoShardSampler); rebuild the 1-rank order: video v is
        the (v // world)-th video of rank v % world.  Small host objects (scores, labels, counts) travel; every rank ends
        with the full result, so the best-accuracy bookkeeping of train() is the same everywhere."""
        rank, world, total = shard
        parts = sdist.gather_objects((logits.cpu(), labels.cpu(), list(sv)))
        offs = []
        for lg, lb, s_ in parts:
            o = [0]
            for c in s_:
                o.append(o[-1] + int(c))
            assert o[-1] == lg.shape[0] == lb.shape[0]
            offs.append(o)
        rows_l, rows_t, sv_all = [], [], []
        for v in range(total):
            r, j = v % world, v // world
            lg, lb, s_ = parts[r]
            if offs[r][j + 1] > offs[r][j]:         # zero-row parts (an empty shard's placeholder width) stay out of the cat
                rows_l.append(lg[offs[r][j]:offs[r][j + 1]])
                rows_t.append(lb[offs[r][j]:offs[r][j + 1]])
            sv_all.append(s_[j])
        dev = logits.device
        if not rows_l:
            return logits, labels, sv_all
        return (torch.cat(rows_l, 0).to(dev).contiguous(), torch.cat(rows_t, 0).to(dev).contiguous(), sv_all)


def aggregate_scores(be, scores: torch.Tensor, labels: torch.Tensor, samples_per_video, softmax: bool):
    """(ps, pred per video, #correct videos) through sfk_eval_aggregate; scores (rows, classes) fp32 on the device.
    Videos without clips are skipped, as the reference loops do (train.py:351-362, train_sparse.py:211-228)."""
    dev = scores.device
    seg = [0]
    for s_ in samples_per_video:
        seg.append(seg[-1] + int(s_))
    assert seg[-1] <= scores.shape[0]
    seg_off = torch.tensor(seg, dtype=torch.int32).to(dev)
    nvid = len(samples_per_video)
    ps = torch.empty_like(scores)
    pred = torch.empty(max(nvid, 1), dtype=torch.int32, device=dev)
    correct = torch.zeros(1, dtype=torch.int32, device=dev)
    if nvid > 0:
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
        be.eval_aggregate(scores, labels, seg_off, nvid, softmax, ps, pred, correct)(stream)
    return ps, pred[:nvid], int(correct[0])
